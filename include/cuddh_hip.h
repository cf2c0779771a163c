/*
 * cuddh_hip.h -- C ABI of the MI355X (gfx950) kernel layer.
 *
 * Every entry point is `extern "C"`, takes plain pointers and sizes, returns an
 * int (0 = success, otherwise the hipError_t value) and takes the HIP stream as
 * an opaque `void*` last argument (NULL = the null stream).  All array
 * arguments are DEVICE pointers unless the name starts with `h_`.  Layouts are
 * column major (first index fastest), exactly the layouts the reference's
 * operator classes already hold in their HostDeviceArray members, so that a
 * maintainer can replace the body of each reference `action()` by one call
 * (see INTEGRATION.md).  Citations are relative to the reference repository
 * arotem3/CuDDHelmholtz.
 *
 * None of these functions allocates, frees or synchronises unless its comment
 * says so (safe to capture in a hipGraph).
 */
#ifndef CUDDH_HIP_H
#define CUDDH_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ runtime */

/* Replaces the cudaMalloc/cudaMemset/cudaMemcpy/cudaFree calls of
 * include/HostDeviceArray.hpp:143,189,259-262,269,296-299.  Blocking. */
int cuddh_hip_malloc_zeroed(void **ptr, size_t bytes);
int cuddh_hip_free(void *ptr);
int cuddh_hip_copy_h2d(void *dst, const void *h_src, size_t bytes);
int cuddh_hip_copy_d2h(void *h_dst, const void *src, size_t bytes);
/* the same, queued on `stream` behind the work already there and complete on return (what HostDeviceArray mirrors and the
 * solver's per-step coefficient copies use: the launch stream may be a non-blocking one) */
int cuddh_hip_copy_h2d_on(void *dst, const void *h_src, size_t bytes, void *stream);
int cuddh_hip_copy_d2h_on(void *h_dst, const void *src, size_t bytes, void *stream);
int cuddh_hip_copy_d2d(void *dst, const void *src, size_t bytes, void *stream);
/* include/linalg.hpp:46-48 (zeros -> cudaMemset) */
int cuddh_hip_memset_zero(void *ptr, size_t bytes, void *stream);
int cuddh_hip_stream_sync(void *stream);
int cuddh_hip_device_sync(void);
/* number of visible devices; 0 if there is no GPU (never fails) */
int cuddh_hip_device_count(void);
/* Pinned host memory, asynchronous device -> host copies and events: what the Arnoldi loop needs to fetch a Hessenberg column
 * while the next matrix-vector product is already queued (csrc/src/krylov.cpp; the reference copies with blocking cudaMemcpy,
 * source/linalg.cpp:67-83).  h_dst of copy_d2h_async must come from host_alloc. */
int cuddh_hip_host_alloc(void **ptr, size_t bytes);
int cuddh_hip_host_free(void *ptr);
int cuddh_hip_copy_d2h_async(void *h_dst, const void *src, size_t bytes, void *stream);
int cuddh_hip_event_create(void **ev);
int cuddh_hip_event_record(void *ev, void *stream);
int cuddh_hip_event_sync(void *ev);
int cuddh_hip_event_destroy(void *ev);
/* the calling thread's current device (hipGetDevice), -1 if there is none; the BLAS-1 wrappers key their reduction scratch by it */
int cuddh_hip_current_device(void);
const char *cuddh_hip_error_string(int err);

/* ------------------------------------------------------------------ BLAS-1
 * source/linalg.cpp:51-201.  `ws` is a caller-owned device workspace of at
 * least cuddh_hip_reduce_ws_bytes() bytes used for the two-stage reduction;
 * `result` is a DEVICE scalar (no host sync, no allocation -- the reference
 * allocates, memsets and D2H-copies a scalar per call, source/linalg.cpp:67-83).
 */
size_t cuddh_hip_reduce_ws_bytes(void);
int cuddh_hip_axpby_f64(int n, double a, const double *x, double b, double *y, void *stream);
int cuddh_hip_axpby_f32(int n, float a, const float *x, float b, float *y, void *stream);
/* y <- (sa * *a_dev) * x + b * y with the coefficient read from device memory
 * (lets the modified Gram-Schmidt loop of source/gmres.cpp:167-172 run without
 * a host round trip per dot product). */
int cuddh_hip_axpby_dev_f64(int n, double sa, const double *a_dev, const double *x, double b, double *y, void *stream);
int cuddh_hip_axpby_dev_f32(int n, float sa, const float *a_dev, const float *x, float b, float *y, void *stream);
/* x <- x / *a_dev   (source/gmres.cpp:179 with H(k+1,k) left on the device) */
int cuddh_hip_scal_inv_dev_f64(int n, const double *a_dev, double *x, void *stream);
int cuddh_hip_scal_inv_dev_f32(int n, const float *a_dev, float *x, void *stream);
int cuddh_hip_dot_f64(int n, const double *x, const double *y, double *result, void *ws, void *stream);
int cuddh_hip_dot_f32(int n, const float *x, const float *y, float *result, void *ws, void *stream);
/* result <- sqrt(sum x[i]^2) */
int cuddh_hip_nrm2_f64(int n, const double *x, double *result, void *ws, void *stream);
int cuddh_hip_nrm2_f32(int n, const float *x, float *result, void *ws, void *stream);
/* result <- sum (x[i]-y[i])^2  (square root taken by the caller; source/linalg.cpp:103-137) */
int cuddh_hip_sqdist_f64(int n, const double *x, const double *y, double *result, void *ws, void *stream);
int cuddh_hip_sqdist_f32(int n, const float *x, const float *y, float *result, void *ws, void *stream);
/* One stage of the modified Gram-Schmidt loop of source/gmres.cpp:167-172 in a single launch:
 *   h = sum of the partial sums `pin` left by the previous stage (= <w, vprev>), stored to *hout;
 *   w <- w - h * vprev;   pout <- per-workgroup partial sums of <w, vnext>  (vnext == NULL: <w, w>).
 * vprev == NULL starts a chain (no update, pin/hout ignored).  pin and pout are the two halves of a workspace of
 * cuddh_hip_reduce_ws_bytes() bytes, used alternately.  `finish` turns the <w,w> partials into the norm
 * (*hout = ||w||) and normalises w (source/gmres.cpp:174-179).  Fixed summation order. */
int cuddh_hip_mgs_stage_f64(int n, double *w, const double *vprev, const double *vnext, const double *pin, double *pout, double *hout, void *stream);
int cuddh_hip_mgs_stage_f32(int n, float *w, const float *vprev, const float *vnext, const float *pin, float *pout, float *hout, void *stream);
int cuddh_hip_mgs_finish_f64(int n, double *w, const double *pin, double *hout, void *stream);
int cuddh_hip_mgs_finish_f32(int n, float *w, const float *pin, float *hout, void *stream);
/* Classical Gram-Schmidt against ALL k1 basis vectors V + j ldv (0 <= j < k1 <= 512) in one launch; applied twice it is the
 * CGS2 orthogonalisation of gmres(..., Orthogonalization::cgs2).  A pass does, in this order,
 *   update != 0:  c[j] = sum_{p < ncin} cin[j cstride + p], the same sum in every workgroup;  hout[j] = (hacc ? hacc[j] : 0) + c[j];
 *                 w <- w - sum_j c[j] v_j, per element in ascending j with one fused multiply-add each
 *                 (ncin = 1, cstride = 1: cin holds k1 final coefficients, e.g. behind an all-reduce)
 *   dots == 1:    per-workgroup partial sums of <w, v_j> (of the updated w) for every j, and of <w, w>
 *   dots == 2:    those of <w, w> only (needs update != 0)
 * Partial layout: `pout` is a buffer of cuddh_hip_cgs_ws_bytes(k1) bytes, rows of 1024 scalars of the vectors' type; workgroup b
 * of the g = cuddh_hip_cgs_partials(n) launched writes pout[b] (<w, w>: row 0, what mgs_finish reads as its `pin`) and
 * pout[(1 + j) 1024 + b] (<w, v_j>).  The next pass consumes them with cin = pout + 1024, ncin = g, cstride = 1024.
 * 16-byte accesses when w, V and (for k1 > 1) ldv * sizeof are multiples of 16 bytes, element-wise otherwise.  n == 0 does
 * nothing; k1 outside [1, 512], ldv < n or another combination of update / dots returns hipErrorInvalidValue and launches nothing.
 * cgs_reduce: out[j] = sum of row 1 + j (j < k1), out[k1] = sum of row 0, by the summation routine of the update's prologue
 * (k1 == 0: the <w, w> row alone).  Fixed summation order throughout. */
size_t cuddh_hip_cgs_ws_bytes(int k1);
int cuddh_hip_cgs_partials(int n);
int cuddh_hip_cgs_pass_f64(int n, double *w, const double *V, long long ldv, int k1, int update, int dots, const double *cin, int ncin, long long cstride,
                           const double *hacc, double *hout, double *pout, void *stream);
int cuddh_hip_cgs_pass_f32(int n, float *w, const float *V, long long ldv, int k1, int update, int dots, const float *cin, int ncin, long long cstride,
                           const float *hacc, float *hout, float *pout, void *stream);
int cuddh_hip_cgs_reduce_f64(int n, int k1, const double *partials, double *out, void *stream);
int cuddh_hip_cgs_reduce_f32(int n, int k1, const float *partials, float *out, void *stream);
/* Solution update of an augmented GMRES cycle (gmres(..., GmresOptions{orth, augment > 0})), one launch.  Every operand is a
 * device pointer.  Per element i, d starts at 0 and takes one fused multiply-add per column: coef[j] * V[j ldv + i] for
 * 0 <= j < nv in ascending j, then coef[nv + p] * Z[p ldz + i] for 0 <= p < nz in ascending p.  Then dx[i] = d and
 * x[i] = x[i] + d.  Workgroup b of the cuddh_hip_cgs_partials(n) launched writes its partial sum of d^2 to pout[b]: row 0 of the
 * partial layout above, so cuddh_hip_cgs_reduce_*(n, 0, pout, out) leaves sum d^2 in out[0].  (nv + nz + 3) n scalars move,
 * against 3 (nv + nz) n of the axpby chain on x.  nv >= 1, nz >= 0 (Z is not read then), nv + nz <= 512.
 * 16-byte accesses when x, dx, V, Z and (for more than one column) ldv * sizeof and ldz * sizeof are multiples of 16 bytes,
 * element-wise otherwise; fixed summation order; vectors of 64 MiB and more are streamed with the non-temporal hint.
 * n == 0 does nothing; nv < 1, nz < 0, nv + nz > 512, ldv < n with nv > 1 or ldz < n with nz > 1 returns hipErrorInvalidValue and
 * launches nothing.  dx must not overlap x, V, Z or coef. */
int cuddh_hip_krylov_update_f64(int n, double *x, double *dx, const double *V, long long ldv, int nv, const double *Z, long long ldz, int nz,
                                const double *coef, double *pout, void *stream);
int cuddh_hip_krylov_update_f32(int n, float *x, float *dx, const float *V, long long ldv, int nv, const float *Z, long long ldz, int nz,
                                const float *coef, float *pout, void *stream);
/* Complex arithmetic on SPLIT vectors (gmres(..., GmresOptions{arithmetic = complex})): a vector of 2 h scalars stands for h complex
 * numbers, real parts at [0, h), imaginary parts at [h, 2 h), one allocation.  Every operand is a device pointer.
 * cmgs_stage: mgs_stage with a complex coefficient, one launch.
 *   c = (sum of pin[0 .. g)) + i (sum of pin[1024 .. 1024 + g)), stored to hout[0], hout[1]  (= <vprev, w>, left by the previous stage);
 *   w <- w - c vprev:  w_r -= c_r v_r - c_i v_i,  w_i -= c_r v_i + c_i v_r;
 *   pout[b], pout[1024 + b] <- workgroup b's partial sums of Re, Im <vnext, w> = (v_r w_r + v_i w_i) + i (v_r w_i - v_i w_r).
 * vprev == NULL starts a chain (no update, pin / hout ignored).  vnext == NULL is the finish stage: pout[b] <- partial sums of
 * |w|^2 over all 2 h scalars, pout[1024 + b] <- 0; cuddh_hip_mgs_finish_*(2 h, w, pout, hout) then normalises w as on the real
 * chain (g = cuddh_hip_cgs_partials(2 h) workgroups in both).  pin and pout are the two halves of a workspace of
 * cuddh_hip_cmgs_ws_bytes() bytes, used alternately.  Launches per Arnoldi step: those of the real chain.
 * ckrylov_update: x <- x + sum_j (coef[2 j] + i coef[2 j + 1]) v_j, v_j = V + j ldv, 0 <= j < k1 <= 512, per element in ascending j,
 * one launch; x is read and written once; vectors of 64 MiB and more are streamed with the non-temporal hint.
 * 16-byte accesses when h is a multiple of the 16-byte vector's width and the operands (and, for k1 > 1, ldv * sizeof) are 16-byte
 * aligned; element-wise for the whole vector otherwise (an odd h leaves the imaginary half misaligned).  Fixed summation order.
 * h == 0 does nothing; h < 0, h >= 2^30, k1 outside [1, 512] or ldv < 2 h with k1 > 1 returns hipErrorInvalidValue and launches
 * nothing. */
size_t cuddh_hip_cmgs_ws_bytes(void);
int cuddh_hip_cmgs_stage_f64(int h, double *w, const double *vprev, const double *vnext, const double *pin, double *pout, double *hout, void *stream);
int cuddh_hip_cmgs_stage_f32(int h, float *w, const float *vprev, const float *vnext, const float *pin, float *pout, float *hout, void *stream);
int cuddh_hip_ckrylov_update_f64(int h, double *x, const double *V, long long ldv, int k1, const double *coef, void *stream);
int cuddh_hip_ckrylov_update_f32(int h, float *x, const float *V, long long ldv, int k1, const float *coef, void *stream);
int cuddh_hip_copy_f64(int n, const double *x, double *y, void *stream);
int cuddh_hip_copy_f32(int n, const float *x, float *y, void *stream);
int cuddh_hip_copy_i32(int n, const int *x, int *y, void *stream);
int cuddh_hip_scal_f64(int n, double a, double *x, void *stream);
int cuddh_hip_scal_f32(int n, float a, float *x, void *stream);
int cuddh_hip_fill_f64(int n, double a, double *x, void *stream);
int cuddh_hip_fill_f32(int n, float a, float *x, void *stream);
int cuddh_hip_fill_i32(int n, int a, int *x, void *stream);
/* y[i] (+)= c * p[i] * x[i]; accumulate != 0 selects +=.  x may alias y.
 * source/MassMatrix.cpp:316-334, source/FaceMassMatrix.cpp:303-321 */
int cuddh_hip_diag_scale_f64(int n, int accumulate, double c, const double *p, const double *x, double *y, void *stream);
/* x[i] <- 1 / x[i]   (source/MassMatrix.cpp:276-279) */
int cuddh_hip_reciprocal_f64(int n, double *x, void *stream);

/* ------------------------------------------------------------------ index maps
 * source/H1Space.cpp:189-219 (FaceSpace::restrict / prolong / orth) */
int cuddh_hip_gather_f64(int n, const int *proj, const double *x, double *y, void *stream);      /* y[i]  = x[proj[i]] */
int cuddh_hip_scatter_add_f64(int n, const int *proj, const double *x, double *y, void *stream); /* y[proj[i]] += x[i] */
int cuddh_hip_zero_indexed_f64(int n, const int *proj, double *x, void *stream);                 /* x[proj[i]] = 0 */
/* y[r] = (accumulate ? y[r] : 0) + sum of x[src[k]], k in [off[r], off[r+1]), added in list order (fixed-order replacement of
 * the atomic adds of source/DDH.cpp:303,306) */
int cuddh_hip_csr_sum_f64(int n_rows, const int *off, const int *src, const double *x, double *y, int accumulate, void *stream);
/* Trace exchange of the multi-GPU DDH path (new: the reference is single-GPU).  A slot t stands for entries t and n_half + t
 * of a trace vector v (lambda and mu halves).  pack: buf[i] = v[slot[i]], buf[n + i] = v[n_half + slot[i]] and, with
 * clear != 0, those entries of v are zeroed (they belong to the receiving rank); unpack: the inverse copy. */
int cuddh_hip_trace_pack_f32(int n, int n_half, const int *slot, float *v, float *buf, int clear, void *stream);
int cuddh_hip_trace_pack_f64(int n, int n_half, const int *slot, double *v, double *buf, int clear, void *stream);
int cuddh_hip_trace_unpack_f32(int n, int n_half, const int *slot, const float *buf, float *v, void *stream);
int cuddh_hip_trace_unpack_f64(int n, int n_half, const int *slot, const double *buf, double *v, void *stream);
/* Halo exchange of the partitioned global operator apply (new: the reference is single-GPU; it partitions the operator of
 * examples/Helmholtz.hpp:28-56).  Entries ids[i] and n_half + ids[i] of a local [u; v] vector v travel as the pair
 * (buf[2 i], buf[2 i + 1]): the messages for several neighbours are contiguous pieces of ONE buffer and one launch packs them all.
 * pack: buf <- v at ids and, with clear != 0, those entries of v are zeroed (partial sums handed to the owner).
 * unpack: v at ids <- buf (add == 0: halo values of x arriving from their owners) or v at ids += buf (add != 0: partial sums of y
 * arriving at the owner; ids of one call are distinct, messages from different senders are added in rank order -> reproducible). */
int cuddh_hip_halo_pack_f64(int n, int n_half, const int *ids, double *v, double *buf, int clear, void *stream);
int cuddh_hip_halo_unpack_f64(int n, int n_half, const int *ids, const double *buf, double *v, int add, void *stream);

/* ------------------------------------------------------------------ element operators (fp64)
 * Shapes: P,D (nq,nb); I (nb,nb,n_elem); J (2,2,nq,nq,n_elem); detJ (nq,nq,n_elem);
 * G (3,nq,nq,n_elem); a (nq,nq,n_elem); w (nq). */

/* source/Mesh2D.cpp:173-227 + source/Element.cpp:5-36: the metric arrays of Mesh2D::ElementMetricCollection on the tensor
 * grid of a 1-D rule q (n points), computed on the device from the elements' corners (2, 4, n_elem; counter-clockwise):
 * J (2,2,n,n,n_elem), detJ (n,n,n_elem), x (2,n,n,n_elem); any output may be NULL. */
int cuddh_hip_element_metrics(int n_elem, int n, const double *corners, const double *q, double *J, double *detJ, double *x, void *stream);
/* source/StiffnessMatrix.cpp:5-38  (setup_geometric_factors) */
int cuddh_hip_stiffness_setup(int n_elem, int nq, const double *w, const double *J, double *G, void *stream);
/* source/StiffnessMatrix.cpp:83-205  y[I] += c * S x */
int cuddh_hip_stiffness_apply(int n_elem, int nq, int nb, const double *P, const double *D, const double *G,
                              const int *I, double c, const double *x, double *y, void *stream);
/* source/MassMatrix.cpp:5-67  (init_mass_matrix); coef may be NULL (=1) */
int cuddh_hip_mass_setup(int n_elem, int nq, int nb, const double *coef, const double *detJ, const double *w,
                         const int *I, const double *P, double *a, void *stream);
/* source/MassMatrix.cpp:137-239  y[I] += c * M x */
int cuddh_hip_mass_apply(int n_elem, int nq, int nb, const int *I, const double *P, const double *a, double c,
                         const double *x, double *y, void *stream);
/* source/MassMatrix.cpp:241-280 (init_diag_mass): op <- 1 / lumped mass.  Zero-fills op first. */
int cuddh_hip_diag_mass_setup(int ndof, int n_elem, int nb, const double *coef, const double *detJ, const double *w,
                              const int *I, double *op, void *stream);
/* source/FaceMassMatrix.cpp:5-49; I (nb,n_faces); detJ (nq,n_faces); a (nq,n_faces) */
int cuddh_hip_facemass_setup(int n_faces, int nb, int nq, const double *w, const double *P, const double *detJ,
                             const double *coef, const int *I, double *a, void *stream);
/* source/FaceMassMatrix.cpp:141-223 */
int cuddh_hip_facemass_apply(int n_faces, int nb, int nq, const double *P, const double *a, const int *I, double c,
                             const double *x, double *y, void *stream);
/* source/FaceMassMatrix.cpp:225-255 (init_diag); op must be zero on entry (the reference relies on that too) */
int cuddh_hip_diag_facemass_setup(int ndof, int n_faces, int nb, const double *w, const double *detJ,
                                  const double *coef, const int *I, double *op, void *stream);

/* ------------------------------------------------------------------ fused complex Helmholtz apply
 * One launch pair for  [u;v] -> [Au;Av]  of examples/Helmholtz.hpp:28-56
 * (2 memsets + 11 launches there).  The plan owns patch-ordered copies of the
 * index map and of the metric arrays (layout in DESIGN.md).  create/destroy
 * allocate, copy and synchronise; apply does not.
 *
 * h_I (nb,nb,n_elem) HOST; h_xy optional HOST element centroids (2,n_elem) used
 * only to order elements into compact patches (NULL = keep element order);
 * G_S (3,nqS,nqS,n_elem), a_M (nqM,nqM,n_elem) DEVICE arrays as produced by
 * cuddh_hip_stiffness_setup / cuddh_hip_mass_setup; boundary-face data:
 * h_fI (nb,n_faces) HOST face -> H1 global index (already composed with the
 * FaceSpace projection), h_face_elem (n_faces) HOST element each face belongs to
 * (Edge::elements[0]), a_F (nqF,n_faces) DEVICE from cuddh_hip_facemass_setup.
 * Returns hipErrorNotSupported (801) for (nb,nqS,nqM) combinations without a
 * specialised kernel; callers then use the separate operators.
 */
typedef struct cuddh_helmholtz_plan cuddh_helmholtz_plan;
int cuddh_hip_helmholtz_plan_create(cuddh_helmholtz_plan **plan, int ndof, int n_elem, int nb, const int *h_I,
                                    const double *h_xy, int nqS, const double *h_PS, const double *h_DS,
                                    const double *G_S, int nqM, const double *h_PM, const double *a_M,
                                    int n_faces, const int *h_fI, const int *h_face_elem, int nqF, const double *h_PF,
                                    const double *a_F);
int cuddh_hip_helmholtz_plan_destroy(cuddh_helmholtz_plan *plan);
/* The plan's patch layout alone, built on the host from the same HOST arrays (no device is touched): which elements form a
 * patch of `pe`, the patch-local numbering, colours, border slots and, with fused != 0, the plan-native vector ordering
 * ("Patch layout").  fixed_stride != 0 pads dof_list / slot_of to max_loc entries per patch.  create returns
 * 0, 1 (more than 65,535 local dofs in a patch, or a face dof outside its element's patch) or 801 (a patch needs a 32nd colour).
 * array copies one field to HOST memory and returns its length (count_only != 0: the length only; -1: unknown name):
 * int: perm dof_off dof_list slot_of own_count patch_nel face_off face_id shared_dof shared_off own_off bpos bslot
 * global_of_native; uint32: lidx; uint16: face_lidx; uint8: colour face_col; one long long each: pe n_patches dof_stride max_loc
 * ncol nfcol n_shared n_slots has_native n_owned bstride list_entries owned_entries native_list_entries; three long long:
 * dest_entries (slot_of entries a write-out reads with no rows, rows of 64, rows of 128 owned dofs skipped). */
typedef struct cuddh_patch_layout cuddh_patch_layout;
int cuddh_patch_layout_create(cuddh_patch_layout **layout, int ndof, int n_elem, int nb, const int *h_I, const double *h_xy,
                              int n_faces, const int *h_fI, const int *h_face_elem, int pe, int fused, int fixed_stride);
long long cuddh_patch_layout_array(const cuddh_patch_layout *layout, const char *name, void *h_out, int count_only);
void cuddh_patch_layout_destroy(cuddh_patch_layout *layout);
/* y = [ S u - w^2 M u - w H v ;  -(S v - w^2 M v + w H u) ],  x = [u;v], y = [Au;Av], each of length ndof */
int cuddh_hip_helmholtz_apply(const cuddh_helmholtz_plan *plan, double omega, const double *x, double *y, void *stream);
/* bytes the plan's apply reads+writes per call: actual == 0 the SURVEY 8d formula of the general-geometry layout,
 * 1 as actually laid out, 2 the "affine" figure when the plan found a metric array identical in every element (uniform
 * meshes: one copy read through scalar loads instead of one per element; 0 otherwise).  CUDDH_PLAN_AFFINE=0 in the
 * environment at plan creation keeps the general form (used to measure the general-geometry roofline on a uniform mesh). */
size_t cuddh_hip_helmholtz_plan_bytes(const cuddh_helmholtz_plan *plan, int actual); /* 3: as laid out for the native apply below */
/* Plan-native vector ordering (not in the reference: its vectors are always [u; v] in H1Space numbering).  For solvers that keep
 * their iteration vectors in the plan's own order -- gmres() only needs an operator and inner products, both invariant under a
 * permutation -- a vector z is an array of ndof (u, v) PAIRS ordered [patch 0's owned dofs | patch 1's ... | patch-border dofs],
 * so the apply reads and writes a patch's owned dofs with contiguous 16-byte accesses and no index list.  has_native: 1 when the
 * plan runs the lane form (helm_lane_kernel: n_basis 2-4, large plans); to_native / from_native are the permutation and its
 * inverse (x, y: [u; v] of length 2 ndof; z: 2 ndof doubles); apply_native is cuddh_hip_helmholtz_apply on native vectors
 * (z_in != z_out).  Same arithmetic in the same order per element and per dof: from_native(apply_native(to_native(x))) is
 * bitwise cuddh_hip_helmholtz_apply(x). */
int cuddh_hip_helmholtz_plan_has_native(const cuddh_helmholtz_plan *plan);
int cuddh_hip_helmholtz_to_native(const cuddh_helmholtz_plan *plan, const double *x, double *z, void *stream);
int cuddh_hip_helmholtz_from_native(const cuddh_helmholtz_plan *plan, const double *z, double *y, void *stream);
int cuddh_hip_helmholtz_apply_native(const cuddh_helmholtz_plan *plan, double omega, const double *z_in, double *z_out, void *stream);
/* which kernel instantiation the plan's apply launches, e.g. "helm_lane_kernel<4,5,8,NT=1,UG=0> pe=64" (tests assert
 * the form they mean to exercise; bench.py reports it instead of re-deriving the size rules) */
int cuddh_hip_helmholtz_plan_describe(const cuddh_helmholtz_plan *plan, char *buf, int cap);
/* diagnostic: with CUDDH_HELM_STAMPS=1 in the environment at plan creation the lane-form kernels record 8 phase time stamps
 * (100 MHz constant clock) per patch; this copies those of the last apply to h_out ([n_patches][8]). */
int cuddh_hip_helmholtz_plan_read_stamps(const cuddh_helmholtz_plan *plan, unsigned long long *h_out, int n_patches);

/* The same plan machinery for ONE real operator -- the bandwidth path of StiffnessMatrix::action
 * (source/StiffnessMatrix.cpp:186-205, kind 0, metric = G (3,nq,nq,n_elem)) and MassMatrix::action
 * (source/MassMatrix.cpp:213-239, kind 1, metric = a (nq,nq,n_elem)):  y = [y +] c * Op x  without atomics
 * and without a zero-fill (accumulate != 0 keeps the reference's action(c,x,y) meaning, 0 is action(x,y)).
 * h_D is ignored for kind 1.  Returns hipErrorNotSupported (801) unless 2 <= nb <= 5 and nq is the rule the
 * reference's constructors pick (nb+1; or 1+3nb/2+1 for the weighted mass); callers then use
 * cuddh_hip_stiffness_apply / cuddh_hip_mass_apply.  destroy/bytes: the helmholtz_plan functions. */
int cuddh_hip_operator_plan_create(cuddh_helmholtz_plan **plan, int kind, int ndof, int n_elem, int nb, const int *h_I,
                                   const double *h_xy, int nq, const double *h_P, const double *h_D, const double *metric);
int cuddh_hip_operator_plan_apply(const cuddh_helmholtz_plan *plan, double c, int accumulate, const double *x, double *y,
                                  void *stream);

/* ------------------------------------------------------------------ DDH local solves
 * source/DDH.cpp:15-58 (init_geom_factors): G (3, nb*nb*mx_elems, n_domains) as
 * Real triples (the reference stores float3), from J (2,2,nb,nb,g_elem). */
int cuddh_hip_ddh_geom_setup_f32(int n_domains, int mx_elems, int g_elem, int nb, const int *n_elems, const int *elems,
                                 const double *w, const double *J, float *G, void *stream);
int cuddh_hip_ddh_geom_setup_f64(int n_domains, int mx_elems, int g_elem, int nb, const int *n_elems, const int *elems,
                                 const double *w, const double *J, double *G, void *stream);

/* The same factors straight from the elements' corners ((2, 4, g_elem), counter-clockwise) and the rule's nodes `points`
 * (nb): the bilinear Jacobian of source/Element.cpp:5-36 is evaluated in the kernel (with the arithmetic of
 * cuddh_hip_element_metrics), so the (2,2,nb,nb,g_elem) table of source/Mesh2D.cpp:173-227 is never built. */
int cuddh_hip_ddh_geom_from_corners_f32(int n_domains, int mx_elems, int nb, const int *n_elems, const int *elems, const double *w,
                                        const double *points, const double *corners, float *G, void *stream);
int cuddh_hip_ddh_geom_from_corners_f64(int n_domains, int mx_elems, int nb, const int *n_elems, const int *elems, const double *w,
                                        const double *points, const double *corners, double *G, void *stream);

/* The arrays DDH holds after its constructor (include/DDH.hpp:55-83,
 * source/DDH.cpp:425-608), in the reference's own layouts.  `real` is float for
 * *_f32 and double for *_f64.  All DEVICE pointers. */
typedef struct cuddh_ddh_desc
{
    int g_ndof;      /* global H1 dofs */
    int n_domains;   /* subdomains (one LDS/register-resident local solve each) */
    int n_lambda;    /* 2 * n_shared */
    int nb;          /* n_basis */
    int nel1d;       /* elements per subdomain edge (NEL); mx_elems = nel1d^2 */
    int mx_dof;      /* leading dimension of gI, m, gmi, a */
    int mx_fdof;     /* leading dimension of B, H */
    int nt;          /* time steps per period */
    double omega;
    double dt;
    const int *s_dof;      /* (n_domains) subdomain sizes          EnsembleSpace::sizes  */
    const int *s_fdof;     /* (n_domains) face-space sizes         EnsembleSpace::fsizes */
    const int *B;          /* (mx_fdof, 2, n_domains) read/write lambda slots, -1 = none  source/DDH.cpp:425-440 */
    const int *gI;         /* (mx_dof, n_domains) permuted subdomain dof -> global dof     source/DDH.cpp:486-497 */
    const int *sI;         /* (nb, nb, mx_elems, n_domains) element node -> permuted subdomain dof  :489-509 */
    const void *D;         /* real (nb, nb) GLL differentiation matrix  :523-528 */
    const void *G;         /* real (3, nb*nb*mx_elems, n_domains)       :530-537 */
    const void *m;         /* real (mx_dof, n_domains) lumped subdomain mass  :541-584 */
    const void *gmi;       /* real (mx_dof, n_domains) global inverse lumped mass :559-591 */
    const void *a;         /* real (mx_dof, n_domains) coefficient      :589 */
    const void *H;         /* real (mx_fdof, n_domains) lumped face mass :593-607 */
    const void *wh_filter; /* real (nt+1)   :370-375 */
    const void *cs;        /* real (2nt+1)  :377-386 */
    const void *sn;        /* real (2nt+1) */
} cuddh_ddh_desc;

typedef struct cuddh_ddh_plan cuddh_ddh_plan;
/* Builds the device-side tables the kernels need on top of the descriptor
 * (deterministic owner-gather lists replacing the LDS atomics of
 * source/DDH.cpp:108; structure check for the wave-per-subdomain kernel).
 * Allocates and synchronises.  is_f64 selects the arithmetic type of `desc`.
 * kernel: 0 = auto, 1 = generic (one workgroup per subdomain, LDS),
 *         2 = wave (one wavefront per subdomain, registers + DPP; nb == 4 only),
 *         3 = wave with the DPP reads folded into the FMAs by hand (fp32; what auto picks when it applies),
 *         4 = 3 with the in-lane contractions on the matrix pipe (v_mfma_f32_4x4x1_16b_f32, fp32),
 *         5 = one 16x16 element matrix applied to the 16 elements of a subdomain per sweep with four
 *             v_mfma_f32_16x16x4_f32 (fp32; needs the same metric tensor in every element and no trace dof
 *             (sI < s_fdof) on an element-interior node, both of which plan_create verifies on the device;
 *             what auto picks when it applies, otherwise 3),
 *         6 = n_basis == 8 (2x2 elements, the reference's other supported shape): one wavefront per TWO
 *             subdomains, registers + DPP over the eight lanes of a column octet,
 *         7 = 6 in separable form (fp32): on the rectangles of a uniform mesh the metric is diagonal and a product of
 *             1-D factors, so a sweep needs ONE 8x8 contraction per direction (D^T diag D precomputed) instead of two
 *             (plan_create verifies the geometry; what auto picks for nb == 8 when it applies),
 *         8 = 5 in fp64 (four v_mfma_f64_16x16x4_f64 per sweep, element matrix formed and kept in double; is_f64, nb == 4
 *             and nel1d == 4 only, same two conditions as 5, which plan_create verifies on the device;
 *             on request only: auto keeps fp64 on 3; hipErrorInvalidValue where it does not apply, like 5),
 *         11 = one 8x8-element subdomain per wavefront (nb == 4, nel1d == 8, fp32): kernel 5's element-lane form with one
 *             element per lane, lane = ex + 8 ey; xi neighbours through DPP row shifts, eta neighbours through ds_bpermute.
 *             Needs rectangles like the element-lane form, the element order ex + 8 ey inside every subdomain and no trace
 *             dof on an element-interior node, which plan_create verifies on the device; what auto picks for that shape
 *             when it applies, otherwise 1.
 *         12 = four 4x4-element subdomains per wavefront at nb == 5 (nel1d == 4, fp32): the element-lane form with the 25
 *             nodes of an element in one lane's registers, lane = ex + 4 ey, one subdomain per 16-lane DPP row; both
 *             contractions in-lane with scalar coefficients, xi and eta neighbours through DPP row shifts that stay in the
 *             row.  Needs what 11 needs (rectangles, the element order ex + 4 ey, no trace dof on an element-interior node;
 *             verified here).  One time grid and RK2 only.  Under auto a qualifying plan takes it from the subdomain count
 *             at which it measured faster than kernel 1 (ELEMENT_LANE5_MIN_DOMAINS in src/ddh_resolve.cpp), kernel 1 below.
 *         13 = the element-lane local solves with four 4x4-element subdomains per wavefront that accept per-subdomain time
 *             grids (fp32, nel1d == 4; on request only, never picked by auto).  nb == 4: needs what kernel 5's element-lane
 *             form needs (the element order ex + 4 ey, one metric for all elements, no trace dof on an element-interior
 *             node, rectangles); nb == 5: what 12 needs; anything else is hipErrorInvalidValue.  Without time grids it
 *             launches the code of kernel 5's element-lane form (cuddh_hip_ddh_plan_set_sweep_form(2)), respectively of
 *             kernel 12: the same bits.  After cuddh_hip_ddh_plan_set_time_grids a wavefront marches once per distinct
 *             grid among its (up to) four subdomains: in a pass the rows on the pass's grid load, march and publish, the
 *             others repeat the pass's first subdomain and publish nothing.  A wavefront whose rows hold k grids costs the
 *             sum of those k marches; a full-range apply lists the subdomains by step count, so at most n_grids - 1 of its
 *             wavefronts hold more than one grid, while ranges and caller lists run in the caller's order and pay for
 *             every grid a group of four holds.  RK2 only; cuddh_hip_ddh_plan_set_sweep_form(2 | 3) is refused and
 *             cuddh_hip_ddh_plan_sweep_form is 0 (it is not kernel 5); cuddh_hip_ddh_plan_set_owner_rule applies.
 * Subdomains hold nb^2 nel1d^2 <= 1024 element nodes.  Kernel 1 runs every such shape (one thread per element node);
 * kernels 2-8 and 11-13 are refused with hipErrorInvalidValue on any shape but their own. */
int cuddh_hip_ddh_plan_create(cuddh_ddh_plan **plan, const cuddh_ddh_desc *desc, int is_f64, int kernel);
/* Plan for subdomains of ANY element connectivity (subdomains given by element labels; desc->nel1d is ignored and
 * should be 0).  mx_elems: elements per subdomain at most, the third extent of desc->sI and the stride of desc->G;
 * nb*nb*mx_elems <= 256.  Element nodes past a subdomain's elements have sI == -1.  The plan builds, once and on the host,
 * the assembly lists in CSR form: for each subdomain dof the element nodes that contribute to it, in ascending element-node
 * order (the summation order of kernel 1), with no cap on how many elements meet at a node.  Tables the plan cannot hold
 * (an sI entry out of range, a dof no element node maps to, sizes past the leading dimensions) are rejected here with
 * hipErrorInvalidValue, never inside a kernel.  Allocates and synchronises.
 * kernel: 0 = auto (9 when nb == 4 and mx_elems <= 16, else 10),
 *         9 = one wavefront per subdomain (nb == 4, <= 16 elements): kernel 3's element-local part (DPP quad contractions;
 *             folded into v_fmac_f32_dpp in fp32), assembly through wave-private LDS along the CSR lists,
 *         10 = one workgroup per subdomain (kernel 1's LDS scheme) summing along the CSR lists (any 2 <= nb <= 10).
 * Kernels 1-8 are not available on a general plan (hipErrorInvalidValue).  The apply entry points below take general
 * plans unchanged. */
int cuddh_hip_ddh_plan_create_general(cuddh_ddh_plan **plan, const cuddh_ddh_desc *desc, int mx_elems, int is_f64, int kernel);
int cuddh_hip_ddh_plan_destroy(cuddh_ddh_plan *plan);
/* which kernel the plan resolved to (1..13) */
int cuddh_hip_ddh_plan_kernel(const cuddh_ddh_plan *plan);
/* Numbering of the forcing x and the solution y of the NEXT apply calls: d_gI (mx_dof, n_domains) DEVICE replaces desc.gI and
 * g_ndof replaces desc.g_ndof for x and y (NULL restores the descriptor's).  With the identity numbering
 * gI(l, s) = l + mx_dof s every subdomain dof has its own entry, so the partition-of-unity contributions that source/DDH.cpp:298-307
 * adds with atomics land in distinct places and can be summed per global dof in a FIXED order afterwards
 * (cuddh_hip_csr_sum_f64): DDH::postprocess is then bitwise reproducible. */
int cuddh_hip_ddh_plan_set_vector_layout(cuddh_ddh_plan *plan, const int *d_gI, int g_ndof);
/* Issue priority of the wavefronts of the NEXT apply calls (s_setprio 3 when high != 0; 0 restores the default).  For the
 * multi-GPU schedule that solves the subdomains feeding other ranks on a second stream: with equal priority they finish
 * together with everything else resident on the device (profiles/r02/overlap_timeline.txt).  Results are unaffected. */
int cuddh_hip_ddh_plan_set_wave_priority(cuddh_ddh_plan *plan, int high);
/* WaveHoltz iterations per local solve.  The reference hard-wires 5 (`constexpr int wh_maxit = 5`,
 * source/DDH.cpp:136) and that is the default; 0 restores it.  A verification knob: with more iterations the local
 * solves become exact and DDH converges to the Helmholtz system its transmission conditions imply
 * (tests/test_ddh_physics.py); production callers never touch it. */
int cuddh_hip_ddh_plan_set_wh_iters(cuddh_ddh_plan *plan, int wh_iters);
/* How a kernel-5 plan forms its stiffness sweep, for every launch of the plan (rhs, action, postprocess, listed and priority
 * launches alike; never a property of one launch, so differently partitioned launches stay bitwise equal):
 *   1 = matrix form: the dense 16x16 element matrix on v_mfma_f32_16x16x4_f32, one subdomain per wavefront;
 *   2 = element-lane form: the separable sweep with one element per lane and four subdomains per wavefront, in-lane FMAs with
 *       scalar coefficients, DPP row shifts for the assembly.  Needs rectangles (diagonal metric, a product of 1-D factors,
 *       the same node weight on both sides of every shared edge), checked when the plan is created;
 *   3 = form 2 with the owner rule turned round: of the 2 or 4 copies of a node that elements share, the one with the largest
 *       element-node index writes the result, not the one with the smallest.  The copies are bitwise equal by construction, so
 *       the results are those of form 2; the value exists so that a test can assert it, and auto never takes it;
 *   0 = auto (the default): 2 when the geometry qualifies and the plan has enough subdomains to fill the device, else 1.
 * 2 or 3 on a plan that is not kernel 5 or does not qualify is refused with hipErrorInvalidValue; 0 and 1 are accepted by
 * every plan.  cuddh_hip_ddh_plan_sweep_form returns the form in effect (1, 2 or 3), 0 for a plan that is not kernel 5. */
int cuddh_hip_ddh_plan_set_sweep_form(cuddh_ddh_plan *plan, int form);
int cuddh_hip_ddh_plan_sweep_form(const cuddh_ddh_plan *plan);
/* The summation order of the element-lane form's in-lane products (forms 2 and 3 of kernel 5), for every launch of the plan:
 *   1 = pinned: every node runs the chain of the node-by-node loop, bit for bit (8 to 10 instructions per register pair);
 *   2 = paired: t = Dg w rounded, then for j = 0..3 the x-term (j != k) and the y-term (j outside the pair's own two rows), last
 *       the two y-terms that read the pair itself as one instruction with the halves crossed: both halves of a pair meet every
 *       term at the same place, 7 packed instructions per pair.  The same terms and the same number of roundings per node in
 *       another order: results differ from order 1 in the last bits;
 *   0 = auto (the default): 2 where auto chose the element-lane form, 1 where cuddh_hip_ddh_plan_set_sweep_form(2 | 3) forced it.
 * 2 is refused with hipErrorInvalidValue, the plan unchanged, on a plan that is not kernel 5, has no element-lane tables, or has
 * time grids or the RK4 integrator (kernel 13 included); on a plan whose form is 1 it is accepted and takes effect when the form
 * becomes 2 or 3 (a plan that takes time grids or RK4 afterwards runs the matrix form, where the order has no effect).  Other values
 * than 0, 1, 2 are invalid.  cuddh_hip_ddh_plan_chain_order returns the order in effect (1 or 2),
 * 0 where the element-lane form is not in effect. */
int cuddh_hip_ddh_plan_set_chain_order(cuddh_ddh_plan *plan, int order);
int cuddh_hip_ddh_plan_chain_order(const cuddh_ddh_plan *plan);
/* Where the element-lane form's march applies the trace sources, for every launch of the plan.  A WaveHoltz pass is affine in
 * its start value, X' = Pi X + r, and r, what the sources contribute, is the same in every pass and is exactly what the first
 * pass (from 0) returns:
 *   1 = every pass computes c(t) F + s(t) Gf in both half steps, as the other kernels do;
 *   2 = the first pass only: the later ones run a time loop without source terms and add the first pass's result behind it
 *       (24 of 228 vector instructions per wavefront-step fewer in four of five passes; r rests in LDS between the time loops).
 *       The same operator Pi and the same sources, rounded at another place: results differ from 1 in the last bits, and are
 *       bitwise those of 1 with one WaveHoltz iteration.  Built beside the paired chains (chain order 2) only;
 *   0 = auto (the default): 2 where the sweep form and the chain order are auto as well and auto gave the paired chains, else 1.
 * 2 is refused with hipErrorInvalidValue, the plan unchanged, exactly where chain order 2 is refused; where it is accepted and the
 * chain order in effect is not 2 it waits, as an order waits on the matrix form.  Other values than 0, 1, 2 are invalid.
 * cuddh_hip_ddh_plan_forcing returns the forcing in effect (1 or 2), 0 where the chain order in effect is not 2. */
int cuddh_hip_ddh_plan_set_forcing(cuddh_ddh_plan *plan, int forcing);
int cuddh_hip_ddh_plan_forcing(const cuddh_ddh_plan *plan);
/* How the march with the sources in the first pass only (forcing 2) carries the velocity q, for every launch of the plan:
 *   1 = as it is: q, with dq = -Hi q + z and qh = q + hm dq formed behind the first sweep of a step (hm = half_dt invm);
 *   2 = scaled: the state is q / (2 hm), the chain of the first sweep opens on 2 (1 - hm Hi) q / (2 hm) / m instead of a bare
 *       product and its assembled result is qh / hm (m: the copies of a shared node inside the subdomain, whose chains the
 *       assembly sums); 6 packed instructions per wavefront-step fewer in every pass.  The same scheme, rounded at other
 *       places: results differ from 1 in the last bits, with one WaveHoltz iteration too;
 *   0 = auto (the default): 2 where sweep form, chain order and forcing are all auto and auto gave forcing 2, else 1.
 * 2 is refused with hipErrorInvalidValue, the plan unchanged, exactly where forcing 2 is refused; where it is accepted and the
 * forcing in effect is not 2 it waits.  Other values than 0, 1, 2 are invalid.  cuddh_hip_ddh_plan_march returns the march in
 * effect (1 or 2), 0 where the forcing in effect is not 2. */
int cuddh_hip_ddh_plan_set_march(cuddh_ddh_plan *plan, int march);
int cuddh_hip_ddh_plan_march(const cuddh_ddh_plan *plan);
/* What the scaled march (march 2) carries as the velocity, for every launch of the plan:
 *   1 = qs = q / (2 hm); the head of the first sweep's chain, alpha / m qs, is multiplied out in every step;
 *   2 = Y = alpha / m qs itself, the same float in all m copies of a node: the chain opens on the state, one packed instruction
 *       per pair and step less (the interior pairs carry 2 qs and keep their bits), the update is Y = fma(alpha / m, z, Y), and
 *       v = Y c / (alpha / m) (2 / dt) is formed once at the end.  The same scheme, rounded at other places: results differ
 *       from 1 in the last bits, with one WaveHoltz iteration too;
 *   0 = auto (the default): 2 wherever the march in effect is 2, whether auto chose that march or a setter did; only an
 *       explicit 1 gives the bits march 2 had before this attribute existed.
 * 2 is refused with hipErrorInvalidValue, the plan unchanged, exactly where march 2 is refused; where it is accepted and the
 * march in effect is not 2 it waits.  Other values than 0, 1, 2 are invalid.  cuddh_hip_ddh_plan_head returns the head in
 * effect (1 or 2), 0 where the march in effect is not 2. */
int cuddh_hip_ddh_plan_set_head(cuddh_ddh_plan *plan, int head);
int cuddh_hip_ddh_plan_head(const cuddh_ddh_plan *plan);
/* How the carried march (head 2) forms the neighbour sums of its two sweeps, for every launch of the plan:
 *   1 = one copy of a shared node forms the sum and the other copy takes it: 16 DPP instructions per sweep on the vector pipe;
 *   2 = every copy fetches the other copy's partial sum with ds_swizzle_b32 (the LDS pipe, no LDS storage) and adds it itself;
 *       a lane without the neighbour does not add (xi) or adds 0 times what it fetched (eta): 16 fetches and 8 packed additions
 *       per sweep.  a + b and b + a are the same float, so the results are bit for bit those of 1 as long as every subdomain
 *       of a wavefront stays finite;
 *   0 = auto (the default): 2 on plans of at least 8,192 subdomains, 1 on smaller ones.
 * 2 is refused with hipErrorInvalidValue, the plan unchanged, where the head in effect is not 2; other values than 0, 1, 2 are
 * invalid.  cuddh_hip_ddh_plan_assembly returns the assembly in effect (1 or 2), 0 where the head in effect is not 2. */
int cuddh_hip_ddh_plan_set_assembly(cuddh_ddh_plan *plan, int assembly);
int cuddh_hip_ddh_plan_assembly(const cuddh_ddh_plan *plan);
/* The owner rule of kernels 11, 12 and 13, for every launch of the plan: of the 2 or 4 copies of a node that elements share, the one with the
 * smallest element-node index publishes (last == 0, the default) or the one with the largest (last != 0).  The copies are
 * bitwise equal by construction, so the results are the same; the switch exists so that a test can assert it.  Refused with
 * hipErrorInvalidValue on a plan that is none of kernels 11, 12 and 13. */
int cuddh_hip_ddh_plan_set_owner_rule(cuddh_ddh_plan *plan, int last);
/* The table of the element-lane kernels (5 in the element-lane form, 11, 12 and 13) alone, computed on the host in double from HOST
 * arrays (no device is touched): h_D (nb, nb) the differentiation matrix, h_G (3, nb, nb) the metric tensor (gx, gy, gz) of one
 * element, nb 4 or 5.  h_out receives 5 nb^2 floats [Bx(k,j) at k + nb j | By(l,j) at l + nb j | Dg(k,l) at k + nb l | W | 1 / W]
 * with  S w = W (Dg w + sum_{j != k} Bx(k,j) w(j,l) + sum_{j != l} By(l,j) w(k,j))  for the element's stiffness matrix S, and
 * W on the last node of either direction replaced by that of node 0, the copy it is assembled with.  Returns 0, -1 when the
 * element does not qualify (a metric that is not diagonal or no product of 1-D factors, a weight W that is not positive or
 * differs between the two sides of a shared edge; h_out is not written), 1 (hipErrorInvalidValue) for another nb or a null
 * pointer.  Plan creation calls the same code on the descriptor's D and G. */
int cuddh_element_lane_tables(int nb, const float *h_D, const float *h_G, float *h_out);
/* The rule by which a DDH plan picks its kernel, sweep form and chain order, alone: host code on plain integers (no device is
 * touched), the code plan creation and the setters above call.
 *   nb, nel1d, n_domains, is_f64: the descriptor's; mx_elems > 0: a label-built plan (nel1d is ignored), else 0;
 *   request: the `kernel` argument of plan creation (0 auto);
 *   facts: what plan creation established about the descriptor, a sum of  2 the NB x NEL element structure holds, 4 one metric
 *       for all elements, 8 no trace dof on an element-interior node, 16 the dense element matrix was built (kernels 5, 8),
 *       32 the separable n_basis-8 tables were built (kernel 7), 64 the element-lane tables were built (kernel 5's
 *       element-lane form, kernels 11, 12, 13);
 *   current: the kernel the plan runs now, 0 at plan creation.  A later resolution starts from it, so an auto choice that time
 *       grids or RK4 moved stays moved when the option is taken back;
 *   time_grids, rk4, sweep_form, chain_order: the options the plan holds (the first two as flags);
 *   setting: which of these the call is about to store, 0 none (creation, time grids, integrator), 1 the sweep form, 2 the chain
 *       order, 3 the owner rule: a chain order 2 and an owner rule are refused where they cannot take effect now, but stay when
 *       a later option makes them idle.
 * out[0..2] receive the kernel (1 to 13), the sweep form in effect (0 to 3) and the chain order in effect (0 to 2); out[3] the
 * checks plan creation runs for this shape and request before it decides, in order, four bits each from the lowest up (1
 * structure, 2 one metric, 3 interior nodes, 4 dense matrix, 5 n_basis-8 tables, 6 element-lane tables: facts holds 1 << check),
 * or -1 where the request is refused on this shape whatever the descriptor holds.  Returns 0, or 1 (hipErrorInvalidValue) where
 * the plan or the setter call is refused (out[0..2] are then 0). */
int cuddh_ddh_resolve(int nb, int nel1d, int n_domains, int is_f64, int mx_elems, int request, int facts, int current, int time_grids, int rk4,
                      int sweep_form, int chain_order, int setting, int *out);
/* The same with the forcing a plan holds (cuddh_hip_ddh_plan_set_forcing; 0 auto) and setting 4, the forcing: out[0..2] as above
 * and out[3] the forcing in effect (0 to 2).  Returns 0, or 1 where the plan or the setter call is refused (out[0..3] are then 0). */
int cuddh_ddh_resolve_forcing(int nb, int nel1d, int n_domains, int is_f64, int mx_elems, int request, int facts, int current, int time_grids,
                              int rk4, int sweep_form, int chain_order, int forcing, int setting, int *out);
/* The same with the march a plan holds as well (cuddh_hip_ddh_plan_set_march; 0 auto) and setting 5, the march: out[0..3] as
 * above and out[4] the march in effect (0 to 2).  Returns 0, or 1 where the plan or the setter call is refused (out[0..4] are
 * then 0). */
int cuddh_ddh_resolve_march(int nb, int nel1d, int n_domains, int is_f64, int mx_elems, int request, int facts, int current, int time_grids,
                            int rk4, int sweep_form, int chain_order, int forcing, int march, int setting, int *out);
/* The same with the head a plan holds as well (cuddh_hip_ddh_plan_set_head; 0 auto) and setting 6, the head: out[0..4] as
 * above and out[5] the head in effect (0 to 2).  Returns 0, or 1 where the plan or the setter call is refused (out[0..5] are
 * then 0). */
int cuddh_ddh_resolve_head(int nb, int nel1d, int n_domains, int is_f64, int mx_elems, int request, int facts, int current, int time_grids,
                           int rk4, int sweep_form, int chain_order, int forcing, int march, int head, int setting, int *out);
/* The same with the assembly a plan holds as well (cuddh_hip_ddh_plan_set_assembly; 0 auto) and setting 7, the assembly:
 * out[0..5] as above and out[6] the assembly in effect (0 to 2).  Returns 0, or 1 where the plan or the setter call is refused
 * (out[0..6] are then 0). */
int cuddh_ddh_resolve_assembly(int nb, int nel1d, int n_domains, int is_f64, int mx_elems, int request, int facts, int current, int time_grids,
                               int rk4, int sweep_form, int chain_order, int forcing, int march, int head, int assembly, int setting, int *out);
/* Per-subdomain time grids.  The descriptor holds ONE grid (nt, dt, wh_filter, cs, sn), taken from the mesh alone; the wave
 * speed 1 / a never enters it, and where a < 1 the explicit time stepping runs past its usable range.  Local
 * solves couple through the traces only, so every subdomain may march its WaveHoltz period on a grid of its own: after this
 * call subdomain s runs h_nt[g] steps of h_dt[g] with g = d_grid_of[s], in every later launch of the plan.
 *   n_grids >= 1; h_nt, h_dt: HOST, one entry per grid;
 *   filter, cs, sn: DEVICE, `real` like the descriptor's, the grids' tables one after the other: grid g's filter starts at
 *       the sum of h_nt[j] + 1 over j < g, its cs and sn at the sum of 2 h_nt[j] + 1 (formulas of the descriptor's tables
 *       with nt = h_nt[g], dt = h_dt[g]);
 *   d_grid_of: DEVICE, n_domains ints in [0, n_grids), read back and checked here.
 * The four DEVICE arrays stay the caller's and must outlive the plan, like the descriptor's.  The descriptor's own grid is
 * then unused.  Allocates and synchronises.
 * One subdomain per wavefront or workgroup is what makes the grid uniform where the time loop reads it, so kernels 1, 2, 3,
 * 4, 5 in the matrix form, 8, 11 and a general plan's 9 and 10 run such a plan (instantiations of their own; a plan without
 * grids launches the code it did before).  The kernels that hold several subdomains per wavefront do not: a kernel-5 plan takes the matrix form whatever
 * its size and refuses cuddh_hip_ddh_plan_set_sweep_form(2 | 3); a plan that auto resolved to kernel 6, 7 or 12 becomes kernel 1;
 * a plan created with kernel 6, 7 or 12 on request and one with sweep form 2 or 3 set are
 * refused with hipErrorInvalidValue, as are a grid with nt < 1 or dt <= 0 and an entry of d_grid_of out of range.
 * Kernel 13 (on request) is the exception among them: four subdomains per wavefront, one march per distinct grid among them.
 * An apply over the whole range [0, n_domains) of such a plan runs the subdomains in the order of their step counts,
 * longest first and by index among equals (a list the plan owns), so that the short solves fill the device behind the
 * long ones; sub-ranges and caller lists run in the caller's order.  A subdomain's result depends on nothing else in the
 * launch, so the order changes no bit of it.
 * cuddh_hip_ddh_plan_time_grids returns the number of grids set, 0 for a plan on the descriptor's grid. */
int cuddh_hip_ddh_plan_set_time_grids(cuddh_ddh_plan *plan, int n_grids, const int *h_nt, const double *h_dt, const void *filter,
                                      const void *cs, const void *sn, const int *d_grid_of);
int cuddh_hip_ddh_plan_time_grids(const cuddh_ddh_plan *plan);
/* The integrator of the local solves: scheme 0 = the explicit midpoint rule (RK2, two stiffness sweeps per step; the default, the
 * reference's), 1 = classical RK4, four sweeps per step:
 *     y = (p, q),  f(t; p, q) = (-q, invm (S p - Hi q + c(t) F + s(t) Gf)),
 *     k1 = f(t_{it-1}; y), k2 = f(t_{it-1/2}; y + dt/2 k1), k3 = f(t_{it-1/2}; y + dt/2 k2), k4 = f(t_it; y + dt k3),
 *     y += dt/6 (k1 + 2 k2 + 2 k3 + k4),  then the filter sums as for RK2.
 * Restart, filter, tables (cs / sn hold every half step), load and publish, wh_iters, priority, lists and ranges and
 * per-subdomain time grids are those of RK2.  The grid is whatever the descriptor (or cuddh_hip_ddh_plan_set_time_grids) holds:
 * RK4 is meant for a grid 2 to 16 times coarser than the mesh grid RK2 needs; the caller builds that grid.
 * RK4 forms exist of kernels 1, 2, 5 (matrix form), 8, 9 and 10 (instantiations of their own; an RK2 plan launches the code it did
 * before).  Like cuddh_hip_ddh_plan_set_time_grids this moves an auto choice and never a request: a plan that auto resolved
 * to kernel 3 becomes kernel 2, one that resolved to 6, 7, 11 or 12 becomes kernel 1, a kernel-5 plan takes the matrix form
 * whatever its size and refuses cuddh_hip_ddh_plan_set_sweep_form(2 | 3); a plan created with kernel 3, 4, 6, 7, 11, 12 or 13 on
 * request and one with sweep form 2 or 3 set are refused with hipErrorInvalidValue and stay
 * RK2 plans; a general plan keeps its kernel, 9 or 10.  No launch of an RK4 plan ever runs RK2 code: a kernel without an RK4 form returns hipErrorInvalidValue.
 * cuddh_hip_ddh_plan_integrator returns the scheme in effect. */
int cuddh_hip_ddh_plan_set_integrator(cuddh_ddh_plan *plan, int scheme);
int cuddh_hip_ddh_plan_integrator(const cuddh_ddh_plan *plan);

/* source/DDH.cpp:111-321 (ddh_action + stiffness).  x: forcing [F;G] (2*g_ndof
 * doubles) or NULL; y: solution output [u;v] (2*g_ndof doubles, zero-filled by
 * the call) or NULL; lambda: traces (2*n_lambda) or NULL; update: outgoing
 * traces (2*n_lambda) or NULL.  Only subdomains [dom_begin, dom_end) are solved
 * (the whole range for a single GPU; a rank's shard for the multi-GPU path).
 * If y != NULL and zero_y != 0 the call zero-fills y first (source/DDH.cpp:144).
 */
int cuddh_hip_ddh_apply_f32(const cuddh_ddh_plan *plan, int dom_begin, int dom_end, const double *x, double *y,
                            int zero_y, const float *lambda, float *update, void *stream);
int cuddh_hip_ddh_apply_f64(const cuddh_ddh_plan *plan, int dom_begin, int dom_end, const double *x, double *y,
                            int zero_y, const double *lambda, double *update, void *stream);
/* The same for the n subdomains listed in d_domains (DEVICE, each in [0, n_domains), no duplicates: the caller's contract) in
 * ONE launch -- the subdomains of a rank whose traces other ranks wait for are not a contiguous range (two block rows of a
 * strip, the rim of a 2-D rank grid), and launching them piecewise leaves pieces running alone on an almost idle device. */
int cuddh_hip_ddh_apply_list_f32(const cuddh_ddh_plan *plan, const int *d_domains, int n, const double *x, double *y, int zero_y,
                                 const float *lambda, float *update, void *stream);
int cuddh_hip_ddh_apply_list_f64(const cuddh_ddh_plan *plan, const int *d_domains, int n, const double *x, double *y, int zero_y,
                                 const double *lambda, double *update, void *stream);

/* ------------------------------------------------------------------ whole-domain WaveHoltz march: stage kernels
 * csrc/kernels/waveholtz.hip, DESIGN 4.5.  One launch does everything a Runge-Kutta sweep does besides its stiffness apply
 * w = K p'; every vector of n doubles is read once and written once.  With
 *     fq(w, q) = invm * (w - Hi * q + c * F + s * G)
 * (c, s: cs[k], sn[k] of the sweep's time; F, G: the load, both NULL for the homogeneous form, which then reads neither):
 *   begin:  p = zu,  q = zv,  u = filt0 zu,  v = filt0 zv
 *   rk2_a:  qh = q + half_dt fq(w, q),   ph = p - half_dt q                                    (w = K p)
 *   rk2_b:  p -= dt qh,  q += dt fq(w, qh),  u += filt p,  v += filt q   (the new p, q)         (w = K ph)
 *   rk4_1:  k = fq(w, q);   ps = p - half_dt q,   qs = q + half_dt k,  aq = k,     ap = -q       (w = K p)
 *   rk4_2:  k = fq(w, qs);  ps = p - half_dt qs,  qs = q + half_dt k,  aq += 2 k,  ap -= 2 qs    (w = K ps; the old qs on the right)
 *   rk4_3:  rk4_2 with dt in the place of half_dt
 *   rk4_4:  k = fq(w, qs);  p += sixth_dt (ap - qs),  q += sixth_dt (aq + k),  u += filt p,  v += filt q
 * Outputs that are also inputs (p, q, u, v, qs, aq, ap) are updated in place; no other two arguments may overlap.  Every
 * product-sum is one fused multiply-add, in the order written.  16-byte accesses when every pointer is 16-byte aligned, element
 * by element otherwise. */
int cuddh_hip_wave_stage_begin_f64(int n, double filt0, const double *zu, const double *zv, double *p, double *q, double *u, double *v,
                                   void *stream);
int cuddh_hip_wave_stage_rk2_a_f64(int n, double half_dt, double c, double s, const double *w, const double *p, const double *q,
                                   const double *invm, const double *Hi, const double *F, const double *G, double *qh, double *ph,
                                   void *stream);
int cuddh_hip_wave_stage_rk2_b_f64(int n, double dt, double c, double s, double filt, const double *w, const double *qh, const double *invm,
                                   const double *Hi, const double *F, const double *G, double *p, double *q, double *u, double *v,
                                   void *stream);
int cuddh_hip_wave_stage_rk4_1_f64(int n, double half_dt, double c, double s, const double *w, const double *p, const double *q,
                                   const double *invm, const double *Hi, const double *F, const double *G, double *ps, double *qs,
                                   double *aq, double *ap, void *stream);
int cuddh_hip_wave_stage_rk4_2_f64(int n, double half_dt, double c, double s, const double *w, const double *p, const double *q,
                                   const double *invm, const double *Hi, const double *F, const double *G, double *ps, double *qs,
                                   double *aq, double *ap, void *stream);
int cuddh_hip_wave_stage_rk4_3_f64(int n, double dt, double c, double s, const double *w, const double *p, const double *q,
                                   const double *invm, const double *Hi, const double *F, const double *G, double *ps, double *qs,
                                   double *aq, double *ap, void *stream);
int cuddh_hip_wave_stage_rk4_4_f64(int n, double sixth_dt, double c, double s, double filt, const double *w, const double *qs,
                                   const double *aq, const double *ap, const double *invm, const double *Hi, const double *F,
                                   const double *G, double *p, double *q, double *u, double *v, void *stream);

/* ------------------------------------------------------------------ whole-domain WaveHoltz march: lattice sweeps
 * csrc/kernels/wave_lattice.hip, DESIGN 4.5.  On a uniform rectangle mesh of nx x ny elements the collocated stiffness is
 *     K = cx diag(Wy) (x) Ax + cy Ay (x) diag(Wx)        on the lattice of Lx x Ly nodes, L = n (n_basis - 1) + 1,
 * Ax, Ay: the 1-D element matrix A assembled along a row of elements that overlap in one node, Wx, Wy: the weights w assembled
 * the same way.  One launch computes w = K p' at every node AND does the stage above: the entry points are the stages' with the
 * stencil's input p' in the place of w (rk2_a and rk4_1 read p once: it is both), and n replaced by the lattice.
 *
 * Vectors hold node (I, J) at I + stride J and have stride * Ly doubles; stride >= Lx and even, every pointer 16-byte aligned.
 * The columns from Lx on are padding: the caller keeps zero state, zero load and invm = 0 there, the kernels keep them zero and
 * the stencil never reads them.  (K p')(I, J) = fma(cx Wy(J), sx, (cy Wx(I)) sy), where sx = sum_d Tx(I, d) p'(I + d, J) and
 * sy = sum_d Ty(J, d) p'(I, J + d) run from zero over ascending d by fused multiply-adds.  With H = n_basis - 1 and k = I mod H:
 * an element-interior node takes d in [-k, H - k] with A[k][k + d]; an element-boundary node d in [-H, H] with A[H][H + d] for
 * d < 0, A[H][H] + A[0][0] for d = 0 and A[0][d] for d > 0; the first and the last node of a line only the side that exists.
 * W is w[k], w[H] + w[0] where two elements meet, w[0] / w[H] at the two ends.  The order depends on (I, J) alone: results are
 * bitwise reproducible, and exact for integer tables.  A is row-major and need not be symmetric.
 * The stencil's input must not be an output (rk4_2 and rk4_3 therefore take ps_in and ps_out); the other inputs may be updated
 * in place as in the stage kernels.  A bad description, a misaligned or NULL pointer, F without G or an output that is the
 * stencil's input return hipErrorInvalidValue (1) and nothing is launched. */
typedef struct cuddh_wave_lattice
{
    int nx, ny, n_basis, stride; /* n_basis in [2, 8] */
    double cx, cy;               /* hy / hx, hx / hy */
    double A[64], w[8];          /* HOST tables: A[k * n_basis + j], w[k] */
} cuddh_wave_lattice;
int cuddh_hip_wave_lattice_rk2_a_f64(const cuddh_wave_lattice *lattice, double half_dt, double c, double s, const double *p, const double *q,
                                     const double *invm, const double *Hi, const double *F, const double *G, double *qh, double *ph,
                                     void *stream);
int cuddh_hip_wave_lattice_rk2_b_f64(const cuddh_wave_lattice *lattice, double dt, double c, double s, double filt, const double *ph,
                                     const double *qh, const double *invm, const double *Hi, const double *F, const double *G, double *p,
                                     double *q, double *u, double *v, void *stream);
int cuddh_hip_wave_lattice_rk4_1_f64(const cuddh_wave_lattice *lattice, double half_dt, double c, double s, const double *p, const double *q,
                                     const double *invm, const double *Hi, const double *F, const double *G, double *ps, double *qs,
                                     double *aq, double *ap, void *stream);
int cuddh_hip_wave_lattice_rk4_2_f64(const cuddh_wave_lattice *lattice, double half_dt, double c, double s, const double *ps_in,
                                     const double *p, const double *q, const double *invm, const double *Hi, const double *F,
                                     const double *G, double *ps_out, double *qs, double *aq, double *ap, void *stream);
int cuddh_hip_wave_lattice_rk4_3_f64(const cuddh_wave_lattice *lattice, double dt, double c, double s, const double *ps_in, const double *p,
                                     const double *q, const double *invm, const double *Hi, const double *F, const double *G,
                                     double *ps_out, double *qs, double *aq, double *ap, void *stream);
int cuddh_hip_wave_lattice_rk4_4_f64(const cuddh_wave_lattice *lattice, double sixth_dt, double c, double s, double filt, const double *ps,
                                     const double *qs, const double *aq, const double *ap, const double *invm, const double *Hi,
                                     const double *F, const double *G, double *p, double *q, double *u, double *v, void *stream);
/* into lattice order: y[i] = x[dof_of_slot[i]], 0 where dof_of_slot[i] < 0 (padding), i < n; begin is the stage `begin` on the
 * gathered zu, zv */
int cuddh_hip_wave_lattice_gather_f64(int n, const int *dof_of_slot, const double *x, double *y, void *stream);
int cuddh_hip_wave_lattice_begin_f64(int n, double filt0, const int *dof_of_slot, const double *zu, const double *zv, double *p, double *q,
                                     double *u, double *v, void *stream);
/* nodes of a workgroup's tile in x and y (the sizes at which the kernels' paths change) */
int cuddh_hip_wave_lattice_tile_x(void);
int cuddh_hip_wave_lattice_tile_y(void);

/* ------------------------------------------------------------------ whole-domain WaveHoltz march: lattice sweeps in fp32
 * csrc/kernels/wave_lattice_f32.hip, DESIGN 4.5.2.  The lattice sweeps above with state, stencil and stages stored and computed
 * in float: the arguments of the cuddh_hip_wave_lattice_*_f64 entry points with float vectors.  Scalars stay double and are
 * rounded to float once on the host.  The description is the same cuddh_wave_lattice: the host forms the stencil's tables from
 * A and w in double exactly as for the fp64 kernels (an element-boundary node's centre coefficient is the double sum
 * A[H][H] + A[0][0], the weight where two elements meet the double sum w[H] + w[0]) and then rounds every table entry, cx and cy
 * to float.  In float, with fused multiply-adds (fmaf) in the orders stated above:
 *     sx, sy from zero over ascending d;   (K p')(I, J) = fmaf(cx * Wy(J), sx, (cy * Wx(I)) * sy), the two products in float;
 * every stage is the fp64 formula in float; the forced form with F = G = 0 gives the homogeneous bits; results depend on (I, J)
 * only and are bitwise reproducible.
 * Vectors have stride * Ly floats; stride >= Lx and stride % 4 == 0, every pointer 16-byte aligned.  The up to three columns from
 * Lx on are padding as above (zero state, zero load, invm = 0; kept zero, never used by the stencil).  A bad description, a
 * stride that is no multiple of 4 or below Lx, a misaligned or NULL pointer, F without G or an output that is the stencil's input
 * return hipErrorInvalidValue (1) and nothing is launched. */
int cuddh_hip_wave32_rk2_a(const cuddh_wave_lattice *lattice, double half_dt, double c, double s, const float *p, const float *q,
                           const float *invm, const float *Hi, const float *F, const float *G, float *qh, float *ph, void *stream);
int cuddh_hip_wave32_rk2_b(const cuddh_wave_lattice *lattice, double dt, double c, double s, double filt, const float *ph, const float *qh,
                           const float *invm, const float *Hi, const float *F, const float *G, float *p, float *q, float *u, float *v,
                           void *stream);
int cuddh_hip_wave32_rk4_1(const cuddh_wave_lattice *lattice, double half_dt, double c, double s, const float *p, const float *q,
                           const float *invm, const float *Hi, const float *F, const float *G, float *ps, float *qs, float *aq, float *ap,
                           void *stream);
int cuddh_hip_wave32_rk4_2(const cuddh_wave_lattice *lattice, double half_dt, double c, double s, const float *ps_in, const float *p,
                           const float *q, const float *invm, const float *Hi, const float *F, const float *G, float *ps_out, float *qs,
                           float *aq, float *ap, void *stream);
int cuddh_hip_wave32_rk4_3(const cuddh_wave_lattice *lattice, double dt, double c, double s, const float *ps_in, const float *p,
                           const float *q, const float *invm, const float *Hi, const float *F, const float *G, float *ps_out, float *qs,
                           float *aq, float *ap, void *stream);
int cuddh_hip_wave32_rk4_4(const cuddh_wave_lattice *lattice, double sixth_dt, double c, double s, double filt, const float *ps,
                           const float *qs, const float *aq, const float *ap, const float *invm, const float *Hi, const float *F,
                           const float *G, float *p, float *q, float *u, float *v, void *stream);
/* in and out of the fp32 lattice order, one rounding each way: load y[i] = (float) x[dof_of_slot[i]], 0 where dof_of_slot[i] < 0
 * (padding), i < n; begin rounds zu, zv and filt0 and then does the stage `begin` in float; store y[g] = (double) x[slot_of_dof[g]],
 * g < ndof */
int cuddh_hip_wave32_load(int n, const int *dof_of_slot, const double *x, float *y, void *stream);
int cuddh_hip_wave32_begin(int n, double filt0, const int *dof_of_slot, const double *zu, const double *zv, float *p, float *q, float *u,
                           float *v, void *stream);
int cuddh_hip_wave32_store(int ndof, const int *slot_of_dof, const float *x, double *y, void *stream);
/* nodes of a workgroup's tile in x and y */
int cuddh_hip_wave32_tile_x(void);
int cuddh_hip_wave32_tile_y(void);

/* ------------------------------------------------------------------ whole-domain WaveHoltz march: two lattice sweeps per launch
 * csrc/kernels/wave_pair.hip (fp64) and wave_pair_f32.hip (fp32), DESIGN 4.5.3.  The stencil input of the second sweep of a pair
 * is pointwise in vectors that exist before the first one: ph = fma(-half_dt, q, p) in rk2_b and rk4_2, fma(-dt, qs, p) in rk4_4
 * (qs the vector rk4_2 wrote).  One launch therefore stages two tiles, takes two stencils and runs two stages:
 *   rk2     = wave_lattice rk2_a then rk2_b          (c0, s0 of the first, c1, s1 of the second)
 *   rk4_12  = wave_lattice rk4_1 then rk4_2          writes ps2 = fma(-half_dt, qs1, p), qs, aq, ap
 *   rk4_34  = wave_lattice rk4_3 (h = dt) then rk4_4 reads the ps2, qs, aq, ap that rk4_12 wrote; q, u, v are updated in place
 * with the lattice, layout, padding, stencil and stage formulas of the entry points above, operation by operation: the results
 * equal those of the two launches bit for bit.  The scalars the march forms (dt / 2, dt / 6) are arguments of their own.
 * A vector that is read with a halo (p and q in rk2 and rk4_12; ps2, p and qs in rk4_34) is still needed by neighbouring
 * workgroups and cannot be an output: rk2 writes p_out, q_out and rk4_34 writes p_out out of place.  A bad description, a stride
 * that is no multiple of 2 (fp64) or 4 (fp32), a misaligned or NULL pointer, F without G or an output that is read with a halo
 * return hipErrorInvalidValue (1) and nothing is launched. */
int cuddh_hip_wave_pair_rk2_f64(const cuddh_wave_lattice *lattice, double half_dt, double dt, double c0, double s0, double c1, double s1,
                                double filt, const double *p, const double *q, const double *invm, const double *Hi, const double *F,
                                const double *G, double *p_out, double *q_out, double *u, double *v, void *stream);
int cuddh_hip_wave_pair_rk4_12_f64(const cuddh_wave_lattice *lattice, double half_dt, double c0, double s0, double c1, double s1,
                                   const double *p, const double *q, const double *invm, const double *Hi, const double *F, const double *G,
                                   double *ps2, double *qs, double *aq, double *ap, void *stream);
int cuddh_hip_wave_pair_rk4_34_f64(const cuddh_wave_lattice *lattice, double dt, double sixth_dt, double c1, double s1, double c2, double s2,
                                   double filt, const double *ps2, const double *p, const double *qs, const double *aq, const double *ap,
                                   const double *invm, const double *Hi, const double *F, const double *G, double *p_out, double *q,
                                   double *u, double *v, void *stream);
/* nodes of a workgroup's tile in x and y: tile_y holds for n_basis 4 and 5, tile_y_run_time for every other n_basis (whose
 * halo of 7 rows would put two tiles of tile_y rows above 64 KB of LDS) */
int cuddh_hip_wave_pair_tile_x(void);
int cuddh_hip_wave_pair_tile_y(void);
int cuddh_hip_wave_pair_tile_y_run_time(void);
/* the fp32 family: the same arguments with float vectors, scalars rounded to float once on the host (as cuddh_hip_wave32_*) */
int cuddh_hip_wave_pair32_rk2(const cuddh_wave_lattice *lattice, double half_dt, double dt, double c0, double s0, double c1, double s1,
                              double filt, const float *p, const float *q, const float *invm, const float *Hi, const float *F, const float *G,
                              float *p_out, float *q_out, float *u, float *v, void *stream);
int cuddh_hip_wave_pair32_rk4_12(const cuddh_wave_lattice *lattice, double half_dt, double c0, double s0, double c1, double s1, const float *p,
                                 const float *q, const float *invm, const float *Hi, const float *F, const float *G, float *ps2, float *qs,
                                 float *aq, float *ap, void *stream);
int cuddh_hip_wave_pair32_rk4_34(const cuddh_wave_lattice *lattice, double dt, double sixth_dt, double c1, double s1, double c2, double s2,
                                 double filt, const float *ps2, const float *p, const float *qs, const float *aq, const float *ap,
                                 const float *invm, const float *Hi, const float *F, const float *G, float *p_out, float *q, float *u,
                                 float *v, void *stream);
int cuddh_hip_wave_pair32_tile_x(void);
int cuddh_hip_wave_pair32_tile_y(void);

/* ------------------------------------------------------------------ whole-domain WaveHoltz march: lattice sweeps with missing cells
 * csrc/kernels/wave_cells.hip (fp64) and wave_cells_f32.hip (fp32), DESIGN 4.5.4.  The lattice, layout, padding, stages and
 * refusals of cuddh_hip_wave_lattice_*_f64 / cuddh_hip_wave32_*, on a grid whose cells are each present or absent: cell (DEVICE,
 * nx * ny bytes) holds 1 where cell a + nx b exists and 0 where it does not.  K is the sum over the present cells of the
 * element's Kronecker sum, regrouped per node.  With H = n_basis - 1, kx = I mod H, ky = J mod H, each sum from zero over
 * ascending d by fused multiply-adds:
 *   kx = 0:      sL = sum_{d = -H..0} A[H][H + d] p'(I + d, J)  (cell column I / H - 1),  wL = w[H];
 *                sR = sum_{d = 0..H} A[0][d] p'(I + d, J)       (cell column I / H),      wR = w[0];
 *   0 < kx < H:  sR = sum_{d = -kx..H - kx} A[kx][kx + d] p'(I + d, J)  (the one column I / H),  wR = w[kx];  sL = 0, no left column;
 * sB, wB (cell row J / H - 1) and sA, wA (cell row J / H) along y likewise.  p' outside the lattice counts as zero, a column or row
 * outside the grid as absent.  With f_XY = 1 where the cell in column X and row Y is present, 0 where it is absent or there is none:
 *   aB = fma(f_RB, sR, f_LB sL),  aA = fma(f_RA, sR, f_LA sL),  tx = fma(wA, aA, wB aB),
 *   bL = fma(f_LA, sA, f_LB sB),  bR = fma(f_RA, sA, f_RB sB),  ty = fma(wR, bR, wL bL),      (K p')(I, J) = fma(cx, tx, cy ty),
 * and (K p')(I, J) = +0 at a node with no present cell around it (the caller keeps zero state, zero load and invm = 0 there, as in
 * the padding).  The order depends on (I, J) and the flags only: bitwise reproducible, exact for integer tables.  A workgroup whose
 * tile (cuddh_hip_wave_lattice_tile_x by _tile_y nodes, the same in both precisions) has no node in a present cell writes nothing.
 * NULL cell is refused like a NULL vector.  The fp32 family rounds the tables, cx, cy and the scalars once, as cuddh_hip_wave32_*. */
int cuddh_hip_wave_cells_rk2_a_f64(const cuddh_wave_lattice *lattice, const unsigned char *cell, double half_dt, double c, double s,
                                   const double *p, const double *q, const double *invm, const double *Hi, const double *F, const double *G,
                                   double *qh, double *ph, void *stream);
int cuddh_hip_wave_cells_rk2_b_f64(const cuddh_wave_lattice *lattice, const unsigned char *cell, double dt, double c, double s, double filt,
                                   const double *ph, const double *qh, const double *invm, const double *Hi, const double *F, const double *G,
                                   double *p, double *q, double *u, double *v, void *stream);
int cuddh_hip_wave_cells_rk4_1_f64(const cuddh_wave_lattice *lattice, const unsigned char *cell, double half_dt, double c, double s,
                                   const double *p, const double *q, const double *invm, const double *Hi, const double *F, const double *G,
                                   double *ps, double *qs, double *aq, double *ap, void *stream);
int cuddh_hip_wave_cells_rk4_2_f64(const cuddh_wave_lattice *lattice, const unsigned char *cell, double half_dt, double c, double s,
                                   const double *ps_in, const double *p, const double *q, const double *invm, const double *Hi, const double *F,
                                   const double *G, double *ps_out, double *qs, double *aq, double *ap, void *stream);
int cuddh_hip_wave_cells_rk4_3_f64(const cuddh_wave_lattice *lattice, const unsigned char *cell, double dt, double c, double s,
                                   const double *ps_in, const double *p, const double *q, const double *invm, const double *Hi, const double *F,
                                   const double *G, double *ps_out, double *qs, double *aq, double *ap, void *stream);
int cuddh_hip_wave_cells_rk4_4_f64(const cuddh_wave_lattice *lattice, const unsigned char *cell, double sixth_dt, double c, double s, double filt,
                                   const double *ps, const double *qs, const double *aq, const double *ap, const double *invm, const double *Hi,
                                   const double *F, const double *G, double *p, double *q, double *u, double *v, void *stream);
int cuddh_hip_wave_cells32_rk2_a(const cuddh_wave_lattice *lattice, const unsigned char *cell, double half_dt, double c, double s, const float *p,
                                 const float *q, const float *invm, const float *Hi, const float *F, const float *G, float *qh, float *ph,
                                 void *stream);
int cuddh_hip_wave_cells32_rk2_b(const cuddh_wave_lattice *lattice, const unsigned char *cell, double dt, double c, double s, double filt,
                                 const float *ph, const float *qh, const float *invm, const float *Hi, const float *F, const float *G, float *p,
                                 float *q, float *u, float *v, void *stream);
int cuddh_hip_wave_cells32_rk4_1(const cuddh_wave_lattice *lattice, const unsigned char *cell, double half_dt, double c, double s, const float *p,
                                 const float *q, const float *invm, const float *Hi, const float *F, const float *G, float *ps, float *qs,
                                 float *aq, float *ap, void *stream);
int cuddh_hip_wave_cells32_rk4_2(const cuddh_wave_lattice *lattice, const unsigned char *cell, double half_dt, double c, double s,
                                 const float *ps_in, const float *p, const float *q, const float *invm, const float *Hi, const float *F,
                                 const float *G, float *ps_out, float *qs, float *aq, float *ap, void *stream);
int cuddh_hip_wave_cells32_rk4_3(const cuddh_wave_lattice *lattice, const unsigned char *cell, double dt, double c, double s, const float *ps_in,
                                 const float *p, const float *q, const float *invm, const float *Hi, const float *F, const float *G,
                                 float *ps_out, float *qs, float *aq, float *ap, void *stream);
int cuddh_hip_wave_cells32_rk4_4(const cuddh_wave_lattice *lattice, const unsigned char *cell, double sixth_dt, double c, double s, double filt,
                                 const float *ps, const float *qs, const float *aq, const float *ap, const float *invm, const float *Hi,
                                 const float *F, const float *G, float *p, float *q, float *u, float *v, void *stream);

/* ------------------------------------------------------------------ whole-domain WaveHoltz march: lattice sweeps with a per-cell stiffness
 * csrc/kernels/wave_weights.hip (fp64) and wave_weights_f32.hip (fp32), DESIGN 4.5.5: the collocated stiffness of -div(beta grad .),
 * beta constant on each cell.  The arguments, the lattice, layout, padding, stages, refusals and aliasing rules are those of
 * cuddh_hip_wave_cells_* above, with one change: `weight` (DEVICE, nx * ny reals, double in the fp64 family and float in the fp32
 * one, cell (a, b) at a + nx b) in place of the flags.  The stencil is the one stated there, term by term and in that order, with
 * f_XY the weight of the cell in column X and row Y and 0 where there is no such cell; (K p')(I, J) = +0 where all four are zero.
 * With weights in {0, 1} the results are the bits of cuddh_hip_wave_cells_*.  A workgroup whose tile has no node in a cell of
 * non-zero weight writes nothing.  The kernels do not inspect the weights: finiteness and sign are the caller's business.
 * hipErrorInvalidValue before any launch, nothing written: a NULL weight, F / G given singly, a bad description or stride, a vector
 * off 16 bytes, an output equal to the stencil input. */
int cuddh_hip_wave_weights_rk2_a_f64(const cuddh_wave_lattice *lattice, const double *weight, double half_dt, double c, double s,
                                     const double *p, const double *q, const double *invm, const double *Hi, const double *F, const double *G,
                                     double *qh, double *ph, void *stream);
int cuddh_hip_wave_weights_rk2_b_f64(const cuddh_wave_lattice *lattice, const double *weight, double dt, double c, double s, double filt,
                                     const double *ph, const double *qh, const double *invm, const double *Hi, const double *F, const double *G,
                                     double *p, double *q, double *u, double *v, void *stream);
int cuddh_hip_wave_weights_rk4_1_f64(const cuddh_wave_lattice *lattice, const double *weight, double half_dt, double c, double s,
                                     const double *p, const double *q, const double *invm, const double *Hi, const double *F, const double *G,
                                     double *ps, double *qs, double *aq, double *ap, void *stream);
int cuddh_hip_wave_weights_rk4_2_f64(const cuddh_wave_lattice *lattice, const double *weight, double half_dt, double c, double s,
                                     const double *ps_in, const double *p, const double *q, const double *invm, const double *Hi, const double *F,
                                     const double *G, double *ps_out, double *qs, double *aq, double *ap, void *stream);
int cuddh_hip_wave_weights_rk4_3_f64(const cuddh_wave_lattice *lattice, const double *weight, double dt, double c, double s,
                                     const double *ps_in, const double *p, const double *q, const double *invm, const double *Hi, const double *F,
                                     const double *G, double *ps_out, double *qs, double *aq, double *ap, void *stream);
int cuddh_hip_wave_weights_rk4_4_f64(const cuddh_wave_lattice *lattice, const double *weight, double sixth_dt, double c, double s, double filt,
                                     const double *ps, const double *qs, const double *aq, const double *ap, const double *invm, const double *Hi,
                                     const double *F, const double *G, double *p, double *q, double *u, double *v, void *stream);
int cuddh_hip_wave_weights32_rk2_a(const cuddh_wave_lattice *lattice, const float *weight, double half_dt, double c, double s, const float *p,
                                   const float *q, const float *invm, const float *Hi, const float *F, const float *G, float *qh, float *ph,
                                   void *stream);
int cuddh_hip_wave_weights32_rk2_b(const cuddh_wave_lattice *lattice, const float *weight, double dt, double c, double s, double filt,
                                   const float *ph, const float *qh, const float *invm, const float *Hi, const float *F, const float *G, float *p,
                                   float *q, float *u, float *v, void *stream);
int cuddh_hip_wave_weights32_rk4_1(const cuddh_wave_lattice *lattice, const float *weight, double half_dt, double c, double s, const float *p,
                                   const float *q, const float *invm, const float *Hi, const float *F, const float *G, float *ps, float *qs,
                                   float *aq, float *ap, void *stream);
int cuddh_hip_wave_weights32_rk4_2(const cuddh_wave_lattice *lattice, const float *weight, double half_dt, double c, double s,
                                   const float *ps_in, const float *p, const float *q, const float *invm, const float *Hi, const float *F,
                                   const float *G, float *ps_out, float *qs, float *aq, float *ap, void *stream);
int cuddh_hip_wave_weights32_rk4_3(const cuddh_wave_lattice *lattice, const float *weight, double dt, double c, double s, const float *ps_in,
                                   const float *p, const float *q, const float *invm, const float *Hi, const float *F, const float *G,
                                   float *ps_out, float *qs, float *aq, float *ap, void *stream);
int cuddh_hip_wave_weights32_rk4_4(const cuddh_wave_lattice *lattice, const float *weight, double sixth_dt, double c, double s, double filt,
                                   const float *ps, const float *qs, const float *aq, const float *ap, const float *invm, const float *Hi,
                                   const float *F, const float *G, float *p, float *q, float *u, float *v, void *stream);

/* ------------------------------------------------------------------ whole-domain WaveHoltz march in three dimensions: box sweeps
 * csrc/kernels/wave_box.hip, DESIGN 4.5.6.  On a box of nx x ny x nz congruent brick elements the collocated stiffness is
 *     K = cx Wz (x) Wy (x) Ax  +  cy Wz (x) Ay (x) Wx  +  cz Az (x) Wy (x) Wx
 * on the lattice of Lx x Ly x Lz Gauss-Lobatto nodes, L = n (n_basis - 1) + 1; Ax, Ay, Az: the 1-D element matrix A assembled along
 * a line of elements that overlap in one node, Wx, Wy, Wz: the weights w assembled the same way (both exactly as stated for
 * cuddh_wave_lattice above: row ids, offset ranges, the centre coefficient A[H][H] + A[0][0] and the weight w[H] + w[0] where two
 * elements meet, each formed once on the host in double).  cx = hy hz / (2 hx), cy = hx hz / (2 hy), cz = hx hy / (2 hz).
 * The six entry points are those of cuddh_hip_wave_lattice_*_f64, argument by argument, with this description in the place of
 * the lattice: one launch computes w = K p' at every node and does the stage.
 *
 * Vectors hold node (I, J, K) at I + stride (J + Ly K) and have stride * Ly * Lz doubles (which must fit in an int); stride >= Lx
 * and even, every pointer 16-byte aligned.  The columns from Lx on are padding: zero state, zero load and invm = 0, kept zero by
 * the kernels and never read by the stencil.  With
 *     sx = sum_d Tx(I, d) p'(I + d, J, K),   sy = sum_d Ty(J, d) p'(I, J + d, K),   sz = sum_d Tz(K, d) p'(I, J, K + d),
 * each from zero over the node's ascending offsets d by fused multiply-adds (T and the ranges as for cuddh_wave_lattice), and
 *     ax = cx * (Wy(J) * Wz(K)),   ay = cy * (Wx(I) * Wz(K)),   az = cz * (Wx(I) * Wy(J))      (each product rounded, inner first),
 *     (K p')(I, J, K) = fma(ax, sx, fma(ay, sy, az * sz)).
 * The order depends on (I, J, K) alone: results are bitwise reproducible, exact for integer tables, and the forced form with
 * F = G = 0 gives the homogeneous bits.  A is row-major and need not be symmetric.
 * The stencil's input must not be an output (rk4_2 and rk4_3 take ps_in and ps_out); the other inputs may be updated in place.
 * A bad description (NULL, a count < 1, n_basis outside [2, 8], stride < Lx or odd, stride * Ly * Lz beyond an int), a misaligned
 * or NULL pointer, F without G or an output that is the stencil's input return hipErrorInvalidValue (1) and nothing is launched. */
typedef struct cuddh_wave_box
{
    int nx, ny, nz, n_basis, stride; /* n_basis in [2, 8] */
    double cx, cy, cz;               /* hy hz / (2 hx), hx hz / (2 hy), hx hy / (2 hz) */
    double A[64], w[8];              /* HOST tables: A[k * n_basis + j], w[k] */
} cuddh_wave_box;
int cuddh_hip_wave_box_rk2_a_f64(const cuddh_wave_box *box, double half_dt, double c, double s, const double *p, const double *q,
                                 const double *invm, const double *Hi, const double *F, const double *G, double *qh, double *ph, void *stream);
int cuddh_hip_wave_box_rk2_b_f64(const cuddh_wave_box *box, double dt, double c, double s, double filt, const double *ph, const double *qh,
                                 const double *invm, const double *Hi, const double *F, const double *G, double *p, double *q, double *u,
                                 double *v, void *stream);
int cuddh_hip_wave_box_rk4_1_f64(const cuddh_wave_box *box, double half_dt, double c, double s, const double *p, const double *q,
                                 const double *invm, const double *Hi, const double *F, const double *G, double *ps, double *qs, double *aq,
                                 double *ap, void *stream);
int cuddh_hip_wave_box_rk4_2_f64(const cuddh_wave_box *box, double half_dt, double c, double s, const double *ps_in, const double *p,
                                 const double *q, const double *invm, const double *Hi, const double *F, const double *G, double *ps_out,
                                 double *qs, double *aq, double *ap, void *stream);
int cuddh_hip_wave_box_rk4_3_f64(const cuddh_wave_box *box, double dt, double c, double s, const double *ps_in, const double *p,
                                 const double *q, const double *invm, const double *Hi, const double *F, const double *G, double *ps_out,
                                 double *qs, double *aq, double *ap, void *stream);
int cuddh_hip_wave_box_rk4_4_f64(const cuddh_wave_box *box, double sixth_dt, double c, double s, double filt, const double *ps,
                                 const double *qs, const double *aq, const double *ap, const double *invm, const double *Hi, const double *F,
                                 const double *G, double *p, double *q, double *u, double *v, void *stream);
/* nodes of a workgroup's tile in x, y and z (the sizes at which the kernels' paths change) */
int cuddh_hip_wave_box_tile_x(void);
int cuddh_hip_wave_box_tile_y(void);
int cuddh_hip_wave_box_tile_z(void);
/* The box problem from arrays alone (csrc/src/wave_box.cpp; plain host code, no device is touched).  h_box = {ax, bx, ay, by, az,
 * bz}; h_a: one finite positive coefficient per lattice node, node (I, J, K) at I + Lx (J + Ly K), or NULL for a == 1; face_mask:
 * bit 0..5 = the faces x = ax, x = bx, y = ay, y = by, z = az, z = bz absorbing (the others sound-hard).  Every output may be NULL:
 * desc (stride = Lx rounded up to even); h_dims = {Lx, Ly, Lz, stride}; in UNPADDED lattice order, Lx Ly Lz each:
 *     h_m    = (hx hy hz / 8) Wz(K) Wy(J) Wx(I)                                   the lumped mass,
 *     h_h    = sum over the absorbing faces that contain the node of the lumped face mass: (hy hz / 4) Wz(K) Wy(J) on an x face,
 *              (hx hz / 4) Wz(K) Wx(I) on a y face, (hx hy / 4) Wy(J) Wx(I) on a z face,
 *     h_invm = 1 / (a^2 m),   h_Hi = h a;
 * h_dof_of_slot (stride Ly Lz: the node of a padded slot, -1 for padding) and h_slot_of_dof (Lx Ly Lz).  A count < 1, an empty or
 * inverted interval, n_basis outside [2, 8], a coefficient that is not finite and positive, a face mask outside 6 bits or
 * stride * Ly * Lz beyond an int return nonzero with cuddh_last_error() beginning "WaveHoltz error: box:" and nothing written. */
int cuddh_wave_box_describe(int nx, int ny, int nz, const double *h_box, int n_basis, const double *h_a, int face_mask, cuddh_wave_box *desc,
                            int *h_dims, double *h_m, double *h_h, double *h_invm, double *h_Hi, int *h_dof_of_slot, int *h_slot_of_dof);
/* cuddh_wave_box_describe with rows of a multiple of `row_multiple` elements: 2 (the call above, array for array) or 4 (the fp32
 * sweeps below: stride = Lx rounded up to a multiple of four).  The stride enters desc, h_dims[3], the two slot maps and the int
 * check; h_m, h_h, h_invm and h_Hi do not depend on it.  Any other row_multiple is refused like the rest ("WaveHoltz error: box:",
 * nothing written). */
int cuddh_wave_box_describe_rows(int nx, int ny, int nz, const double *h_box, int n_basis, const double *h_a, int face_mask, int row_multiple,
                                 cuddh_wave_box *desc, int *h_dims, double *h_m, double *h_h, double *h_invm, double *h_Hi, int *h_dof_of_slot,
                                 int *h_slot_of_dof);

/* ------------------------------------------------------------------ the box sweeps in fp32
 * csrc/kernels/wave_box_f32.hip, DESIGN 4.5.7.  The six entry points above with float vectors: the same description, the same
 * stencil and stage arithmetic statement for statement in float (every product-sum an fmaf, sx, sy, sz each from zero over the
 * ascending offsets, ax, ay, az with each product rounded, the inner first, (K p') = fmaf(ax, sx, fmaf(ay, sy, az * sz))), the
 * scalars still double.  The tables built in double from A and w, cx, cy, cz and every scalar of the call are rounded to float
 * once on the host, as for cuddh_hip_wave32_*.  Results depend on (I, J, K) alone: bitwise reproducible, and the forced form with
 * F = G = 0 gives the homogeneous bits.
 * Vectors hold node (I, J, K) at I + stride (J + Ly K) and have stride * Ly * Lz floats (which must fit in an int); stride >= Lx
 * and a MULTIPLE OF 4, every pointer 16-byte aligned, so every row and plane starts on a 16-byte boundary.  The up to three
 * columns from Lx on are padding: zero state, zero load and invm = 0, kept zero by the kernels and never used by the stencil.
 * Vectors enter and leave this layout through cuddh_hip_wave32_load / _begin / _store.
 * A bad description (NULL, a count < 1, n_basis outside [2, 8], stride < Lx or no multiple of 4, stride * Ly * Lz beyond an int), a
 * misaligned or NULL pointer, F without G or an output that is the stencil's input return hipErrorInvalidValue (1) and nothing is
 * launched. */
int cuddh_hip_wave_box32_rk2_a(const cuddh_wave_box *box, double half_dt, double c, double s, const float *p, const float *q,
                               const float *invm, const float *Hi, const float *F, const float *G, float *qh, float *ph, void *stream);
int cuddh_hip_wave_box32_rk2_b(const cuddh_wave_box *box, double dt, double c, double s, double filt, const float *ph, const float *qh,
                               const float *invm, const float *Hi, const float *F, const float *G, float *p, float *q, float *u, float *v,
                               void *stream);
int cuddh_hip_wave_box32_rk4_1(const cuddh_wave_box *box, double half_dt, double c, double s, const float *p, const float *q,
                               const float *invm, const float *Hi, const float *F, const float *G, float *ps, float *qs, float *aq, float *ap,
                               void *stream);
int cuddh_hip_wave_box32_rk4_2(const cuddh_wave_box *box, double half_dt, double c, double s, const float *ps_in, const float *p,
                               const float *q, const float *invm, const float *Hi, const float *F, const float *G, float *ps_out, float *qs,
                               float *aq, float *ap, void *stream);
int cuddh_hip_wave_box32_rk4_3(const cuddh_wave_box *box, double dt, double c, double s, const float *ps_in, const float *p,
                               const float *q, const float *invm, const float *Hi, const float *F, const float *G, float *ps_out, float *qs,
                               float *aq, float *ap, void *stream);
int cuddh_hip_wave_box32_rk4_4(const cuddh_wave_box *box, double sixth_dt, double c, double s, double filt, const float *ps,
                               const float *qs, const float *aq, const float *ap, const float *invm, const float *Hi, const float *F,
                               const float *G, float *p, float *q, float *u, float *v, void *stream);
/* nodes of a workgroup's tile in x, y and z */
int cuddh_hip_wave_box32_tile_x(void);
int cuddh_hip_wave_box32_tile_y(void);
int cuddh_hip_wave_box32_tile_z(void);

#ifdef __cplusplus
}
#endif
#endif /* CUDDH_HIP_H */
