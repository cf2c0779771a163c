/*
 * cuddh_capi.h -- C handle layer over the host-side C++ mirror of the reference
 * API (cuddh::Mesh2D, Basis, H1Space, FaceSpace, EnsembleSpace, the operator
 * classes, DDH, gmres).  It exists so that non-C++ hosts (the Python package,
 * tests, bench.py) drive exactly the objects a C++ user of cuddh.hpp drives.
 * Plain pointers and sizes only.  Unless a comment says HOST, vector arguments
 * are DEVICE pointers.  Functions returning `int` return 0 on success; functions
 * returning a handle return NULL on failure; cuddh_last_error() then holds the
 * message.  Handles are freed with the matching *_destroy.
 */
#ifndef CUDDH_CAPI_H
#define CUDDH_CAPI_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

const char *cuddh_last_error(void);
/* stream used by every subsequent launch of the library (NULL = null stream) */
void cuddh_set_stream(void *stream);
/* the calling thread's current launch stream (NULL = the null stream) */
void *cuddh_get_stream(void);

/* ---- quadrature / basis (reference include/QuadratureRule.hpp, include/Basis.hpp); HOST arrays */
/* type 0 = Gauss-Legendre, 1 = Gauss-Lobatto */
int cuddh_quadrature(int n, int type, double *h_x, double *h_w);
void *cuddh_basis_create(int n);
void cuddh_basis_destroy(void *basis);
int cuddh_basis_eval(void *basis, int m, const double *h_x, double *h_P);  /* P (m, n) */
int cuddh_basis_deriv(void *basis, int m, const double *h_x, double *h_D); /* D (m, n) */

/* ---- mesh (reference include/Mesh2D.hpp) */
void *cuddh_mesh_uniform_rect(int nx, double ax, double bx, int ny, double ay, double by);
/* the cells of cuddh_mesh_uniform_rect(nx, ax, bx, ny, ay, by) whose h_present[i + nx * j] is nonzero (HOST, nx * ny bytes, at
 * least one nonzero), in ascending cell index, with the unused vertices dropped: a grid mesh with missing cells */
void *cuddh_mesh_grid_cells(int nx, double ax, double bx, int ny, double ay, double by, const unsigned char *h_present);
void *cuddh_mesh_from_vertices(int n_pts, const double *h_xy, int n_elem, const int *h_elems);
/* mesh ingestion (csrc/include/cuddh/meshio.hpp): the reference's text format (tests/load_unstructured_square.cpp:11-55),
 * `times` rounds of uniform refinement of an existing mesh, and labels for EnsembleSpace (n_parts compact element sets) */
void *cuddh_mesh_load(const char *dir);
void *cuddh_mesh_refined(void *mesh, int times);
int cuddh_mesh_partition(void *mesh, int n_parts, int *h_labels); /* (n_elem) */
void cuddh_mesh_destroy(void *mesh);
int cuddh_mesh_n_elem(void *mesh);
int cuddh_mesh_n_edges(void *mesh);
int cuddh_mesh_n_nodes(void *mesh);
int cuddh_mesh_n_boundary_edges(void *mesh);
int cuddh_mesh_boundary_edges(void *mesh, int *h_out);
/* h_out[8*e..] = {type (0 interior, 1 boundary), node0, node1, elem0, elem1, side0, side1, delta} for every edge */
int cuddh_mesh_edges(void *mesh, int *h_out);
double cuddh_mesh_min_h(void *mesh);
int cuddh_mesh_vertices(void *mesh, double *h_xy);  /* (n_nodes, 2) */
int cuddh_mesh_elements(void *mesh, int *h_elems);  /* (n_elem, 4) corner node ids, counter-clockwise */

/* ---- spaces (reference include/H1Space.hpp) */
void *cuddh_h1space_create(void *mesh, void *basis);
void cuddh_h1space_destroy(void *fem);
int cuddh_h1space_size(void *fem);
int cuddh_h1space_global_indices(void *fem, int *h_I);  /* (nb, nb, n_elem) */
int cuddh_h1space_coordinates(void *fem, double *h_xy); /* (2, ndof) */
const int *cuddh_h1space_global_indices_device(void *fem);
const double *cuddh_h1space_coordinates_device(void *fem);

void *cuddh_facespace_create(void *fem, int n_faces, const int *h_faces);
void cuddh_facespace_destroy(void *fs);
int cuddh_facespace_size(void *fs);
int cuddh_facespace_subspace_indices(void *fs, int *h_I); /* (nb, n_faces) */
int cuddh_facespace_global_indices(void *fs, int *h_proj); /* (fdof) */
int cuddh_facespace_restrict(void *fs, const double *x, double *y);
int cuddh_facespace_prolong(void *fs, const double *x, double *y);
int cuddh_facespace_orth(void *fs, double *x);

/* ---- EnsembleSpace (reference include/EnsembleSpace.hpp) */
void *cuddh_ensemble_create(void *fem, int n_spaces, const int *h_labels);
void cuddh_ensemble_destroy(void *ens);
/* h_dims = {n_spaces, mx_elems, mx_faces, mx_ndof, mx_fdof, n_shared} */
int cuddh_ensemble_dims(void *ens, int *h_dims);
/* name in {"gI","sizes","elements","n_elems","faces","n_faces","sI","fI","pI","fsizes","cmap"}; copies the whole HOST array */
int cuddh_ensemble_array(void *ens, const char *name, int *h_out);

/* ---- operators (reference include/StiffnessMatrix.hpp, MassMatrix.hpp, FaceMassMatrix.hpp) */
void *cuddh_stiffness_create(void *fem, int nq /* 0: default rule */);
void *cuddh_mass_create(void *fem, const double *coef /* DEVICE nodal coefficient or NULL */);
void *cuddh_diaginv_mass_create(void *fem, const double *coef);
void *cuddh_facemass_create(void *fs, const double *coef /* DEVICE FaceSpace vector or NULL */);
void *cuddh_diaginv_facemass_create(void *fs, const double *coef);
/* fused complex Helmholtz operator (examples/Helmholtz.hpp semantics); a2x H1 nodal, ax FaceSpace values, DEVICE */
void *cuddh_helmholtz_create(double omega, const double *a2x, const double *ax, void *fem, void *fs);
void cuddh_operator_destroy(void *op);
int cuddh_operator_apply(void *op, const double *x, double *y);               /* y = A x */
int cuddh_operator_apply_add(void *op, double c, const double *x, double *y); /* y += c A x */
int cuddh_helmholtz_apply_unfused(void *op, const double *x, double *y);
int cuddh_helmholtz_is_fused(void *op);
/* kernel instantiation the operator's action() launches (Helmholtz, Stiffness, Mass; "generic"/"unfused" otherwise) */
int cuddh_operator_kernel_name(void *op, char *buf, int cap);
/* diagnostic: phase time stamps of the last fused apply, see cuddh_hip_helmholtz_plan_read_stamps */
int cuddh_helmholtz_read_stamps(void *op, unsigned long long *h_out, int n_patches);
size_t cuddh_helmholtz_bytes(void *op, int actual); /* actual: 0 / 1 / 2 / 3 as cuddh_hip_helmholtz_plan_bytes */
/* plan-native vector ordering of the fused operator (cuddh_hip.h: cuddh_hip_helmholtz_apply_native); vectors of 2 * ndof doubles */
int cuddh_helmholtz_has_native(void *op);
int cuddh_helmholtz_to_native(void *op, const double *x, double *z);
int cuddh_helmholtz_from_native(void *op, const double *z, double *y);
int cuddh_helmholtz_apply_native(void *op, const double *z_in, double *z_out);

/* ---- load vectors with built-in integrands (device lambdas cannot cross a C ABI).
 * integrand: 0 two Gaussians of examples/DDH.cpp:61-72 (param = omega)
 *            1 disk coefficient of examples/DDH.cpp:74-83
 *            2 tests/mass.cpp:3-7 polynomial     3 tests/stiffness.cpp:16-22 (-Laplacian)
 *            4 tests/stiffness.cpp:6-11 function  5 constant param    6 square of integrand 1
 * nq = 0: collocated Gauss-Lobatto rule of the basis; otherwise Gauss-Legendre with nq points. */
int cuddh_linear_functional(void *fem, int nq, int integrand, double param, double c, int accumulate, double *F);
int cuddh_face_linear_functional(void *fs, int nq, int integrand, double param, double c, int accumulate, double *F);
/* out[i] = integrand(x_i) at the collocation point of every H1 dof */
int cuddh_nodal_values(void *fem, int integrand, double param, double *out);

/* ---- DDH (reference include/DDH.hpp) */
/* h_a HOST nodal coefficient; f64 != 0 selects the fp64 parity variant (double traces);
 * kernel: 0 auto, 1 workgroup-per-subdomain, 2 wavefront-per-subdomain, 3 wavefront with DPP-folded FMAs */
void *cuddh_ddh_create(double omega, const double *h_a, void *fem, int nx, int ny, int f64, int kernel);
/* the same with subdomains of block x block elements: 0 or 16 / n_basis is cuddh_ddh_create's size; else block >= 1,
 * n_basis^2 block^2 <= 1024, nx and ny multiples of block (checked before anything is allocated; NULL + cuddh_last_error
 * otherwise).  kernel: 0 auto, 1 workgroup-per-subdomain (any block), 11 one 8x8 block per wavefront (n_basis 4, block 8,
 * f64 == 0; what auto picks there); cuddh_ddh_create's other kernels on its block size only.  cuddh_ddh_info reports
 * nel1d = the block in effect. */
void *cuddh_ddh_create_block(double omega, const double *h_a, void *fem, int nx, int ny, int block, int f64, int kernel);
/* subdomains from element labels on any mesh: h_labels HOST (n_elem), label of every element in [0, n_domains), no empty
 * subdomain, at most 256 element nodes per subdomain (checked before anything is allocated; NULL + cuddh_last_error otherwise).
 * kernel: 0 auto, 9 one wavefront per subdomain (n_basis 4, <= 16 elements), 10 one workgroup per subdomain
 * (cuddh_hip_ddh_plan_create_general).  cuddh_ddh_info reports nel1d = 0. */
void *cuddh_ddh_create_labels(double omega, const double *h_a, void *fem, int n_domains, const int *h_labels, int f64, int kernel);
/* cuddh_ddh_create_labels with a time-step policy and an integrator, encoded as in cuddh_ddh_create_integrator: policy 0 mesh,
 * 1 coefficient, 2 h_ratios HOST with n_ratios = n_domains (one ratio per label, each in [1, 256]); integrator 0 = RK2 (coarsen
 * must be 1), 1 = RK4 on ceil(nt_mesh / coarsen) steps, coarsen in [1, 16].  Checked in this order before anything is allocated
 * (NULL + cuddh_last_error): the integrator ("DDH error: integrator"), the labels, the policy ("DDH error: time step").  kernel:
 * 0 / 9 / 10 as in cuddh_ddh_create_labels; both kernels have every form, so auto picks as it does there. */
void *cuddh_ddh_create_labels_integrator(double omega, const double *h_a, void *fem, int n_domains, const int *h_labels, int f64, int kernel,
                                         int policy, const int *h_ratios, int n_ratios, int integrator, int coarsen);
/* cuddh_ddh_create_block with a time-step policy (cuddh::DDHTimeStep): 0 = the mesh grid, cuddh_ddh_create_block itself;
 * 1 = from the coefficient: subdomain s marches r_s times the mesh grid's steps, r_s = max(1, ceil((1 - 1e-9) / min a over its
 * dofs)); one ratio for all gives a plain plan on that grid, several a plan with per-subdomain time grids
 * (cuddh_hip_ddh_plan_set_time_grids); 2 = h_ratios HOST, n_ratios = the number of subdomains, r_s = h_ratios[s], always run
 * per subdomain.  A non-finite or non-positive a (policy 1), a ratio outside [1, 256] and a wrong n_ratios are refused before
 * anything is allocated (NULL + cuddh_last_error, the message starts with "DDH error: time step").  cuddh_ddh_info keeps
 * reporting the base grid (the mesh grid, or the one grid of policy 1 with one ratio). */
void *cuddh_ddh_create_timegrid(double omega, const double *h_a, void *fem, int nx, int ny, int block, int f64, int kernel, int policy,
                                const int *h_ratios, int n_ratios);
/* cuddh_ddh_create_timegrid with an integrator (cuddh::DDHIntegrator): integrator 0 = RK2 on the mesh grid (coarsen must be 1:
 * cuddh_ddh_create_timegrid itself), 1 = classical RK4 on the base grid of ceil(nt_mesh / coarsen) steps, coarsen in [1, 16];
 * the ratios of `policy` multiply that count.  With a == 1 RK4 is stable up to coarsen ~ 23; the range scales with min a over
 * a subdomain unless policy 1 compensates (a = 0.2 under policy 0: coarsen <= 4).  cuddh_ddh_info and cuddh_ddh_table report the
 * coarsened grid.  An unknown integrator, a coarsen outside [1, 16] and coarsen > 1 with RK2 are refused before anything is
 * allocated (NULL + cuddh_last_error, the message starts with "DDH error: integrator"); a kernel without an RK4 form (3, 4, 6,
 * 7, 11 on request) fails on first use. */
void *cuddh_ddh_create_integrator(double omega, const double *h_a, void *fem, int nx, int ny, int block, int f64, int kernel, int policy,
                                  const int *h_ratios, int n_ratios, int integrator, int coarsen);
/* *scheme = 0 (RK2) or 1 (RK4), *coarsen = the factor in effect.  Returns 0, -1 on error. */
int cuddh_ddh_integrator(void *ddh, int *scheme, int *coarsen);
/* h_out HOST (n_domains) or NULL: r_s of every subdomain (all 1 for the mesh grid).  Returns n_domains, -1 on error. */
int cuddh_ddh_time_ratios(void *ddh, int *h_out);
void cuddh_ddh_destroy(void *ddh);
int cuddh_ddh_size(void *ddh);
/* h_info = {n_domains, nt, n_lambda, mx_dof, mx_fdof, nel1d, kernel (needs a GPU; -1 if none), is_f64}; *h_dt = time step */
int cuddh_ddh_info(void *ddh, int *h_info, double *h_dt);
/* ---- DDH over the GPUs of one node from one process (csrc/include/cuddh/multigpu.hpp; RCCL send/recv + all-reduce) */
typedef struct cuddh_multi_gpu_result
{
    int success, num_iter, num_matvec, n_res, world, used_rccl;
    double t_setup, t_rhs, t_gmres, t_postprocess;
    long long bytes_sent_per_action_rank0;
} cuddh_multi_gpu_result;
/* rhs -> gmres -> postprocess of examples/DDH.cpp:141-144 on uniform_rect(nx), Basis(nb), fp32 DDH, `world` devices.
 * h_a (ndof), h_f (2 ndof), h_u (2 ndof) HOST in the global numbering; h_res (maxit + 2) receives the residual history.
 * force_rccl: bits 0-1 = transport (0 RCCL for world > 1, 1 RCCL also for one rank, 2 loopback: ranks are threads sharing
 * device 0, a test transport), bit 2 (value 4) = split schedule (boundary subdomains first on a second stream with issue
 * priority, exchange behind them, interior meanwhile), bits 8-15 / 16-23 = gx / gy of a rank grid (gx gy = world: ranks own
 * rectangles of the subdomain grid; 0 = strips of block rows); csrc/include/cuddh/multigpu.hpp. */
int cuddh_ddh_solve_multi_gpu(int nx, int nb, double omega, const double *h_a, const double *h_f, double *h_u, int world, int m,
                              int maxit, double tol, int force_rccl, cuddh_multi_gpu_result *out, double *h_res);
/* ---- the fused Helmholtz operator (examples/Helmholtz.hpp:28-56) partitioned over the GPUs of one node from one process
 * (csrc/include/cuddh/multigpu.hpp: helmholtz_multi_gpu; partition.hpp).  mesh: a Mesh2D handle; h_a2x (ndof), h_ax (FaceSpace of
 * ALL boundary edges, in increasing edge id), h_x / h_y ([u; v], 2 ndof) HOST, global numbering.  maxit == 0: h_y = A h_x, then
 * `reps` timed applies; maxit > 0: GMRES(m) solve of A y = h_x.  transport: 0 RCCL, 1 RCCL also for one rank, 2 loopback ranks
 * (threads sharing device 0; a test transport). */
typedef struct cuddh_helmholtz_multi_gpu_result
{
    int success, num_iter, num_matvec, n_res, world, used_rccl;
    double t_setup, t_apply, t_gmres;
    long long n_loc_max, n_halo_max, halo_bytes_per_apply_max;
} cuddh_helmholtz_multi_gpu_result;
int cuddh_helmholtz_multi_gpu(void *mesh, int nb, double omega, const double *h_a2x, const double *h_ax, const double *h_x, double *h_y,
                              int world, int transport, int reps, int m, int maxit, double tol, cuddh_helmholtz_multi_gpu_result *out,
                              double *h_res /* maxit + 2 or NULL */);
/* lists of HelmholtzPartition::build for `rank` of `world` (host only): which = 0 my_elems, 1 l2g, 2 owned, 3 halo, 4 own_to[peer],
 * 5 halo_from[peer], 6 face_l2g, 7 faces.  Returns the count (-1 on error); h_out may be NULL to ask for the count only. */
int cuddh_helmholtz_partition_query(void *mesh, void *fem, void *fs, int rank, int world, int which, int peer, int *h_out);
/* ownership / send / receive lists of the trace exchange for `rank` of `world` (host only; what both the C++ and the
 * Python multi-GPU hosts use).  which: 0 owned slots, 1 slots sent to `peer`, 2 slots received from `peer`, 3 / 4 the subdomains
 * of the boundary / interior launch of the split schedule.  Returns the
 * count (-1 on error); h_out may be NULL to ask for the count only.  h_B: (mx_fdof, 2, n_domains). */
int cuddh_trace_exchange_query(const int *h_B, int n_domains, int mx_fdof, int n_lambda, int rank, int world, int which, int peer,
                               int *h_out);
/* verification knob: WaveHoltz iterations per local solve (reference: 5, source/DDH.cpp:136; 0 restores it) */
int cuddh_ddh_set_wh_iters(void *ddh, int n);
/* the local solves launched next take issue priority on the device (cuddh_hip_ddh_plan_set_wave_priority); 0 restores */
int cuddh_ddh_set_wave_priority(void *ddh, int high);
/* kernel 5's sweep form: 0 auto, 1 matrix, 2 element-lane, 3 the same with the other owner rule (cuddh_hip_ddh_plan_set_sweep_form);
 * the getter returns the form in effect (1, 2 or 3; 0 for a plan that is not kernel 5; -1 on error) */
int cuddh_ddh_set_sweep_form(void *ddh, int form);
int cuddh_ddh_sweep_form(void *ddh);
/* the summation order of the element-lane form's in-lane products: 0 auto, 1 pinned, 2 paired (cuddh_hip_ddh_plan_set_chain_order);
 * the getter returns the order in effect (1 or 2; 0 where the element-lane form is not in effect; -1 on error) */
int cuddh_ddh_set_chain_order(void *ddh, int order);
int cuddh_ddh_chain_order(void *ddh);
/* where the element-lane form's march applies the trace sources: 0 auto, 1 in every WaveHoltz pass, 2 in the first pass only
 * (cuddh_hip_ddh_plan_set_forcing); the getter returns the forcing in effect (1 or 2; 0 where the paired chains are not in effect;
 * -1 on error) */
int cuddh_ddh_set_forcing(void *ddh, int forcing);
int cuddh_ddh_forcing(void *ddh);
/* how that march carries the velocity: 0 auto, 1 as it is, 2 scaled, with its midpoint update folded into the sweep
 * (cuddh_hip_ddh_plan_set_march); the getter returns the march in effect (1 or 2; 0 where forcing 2 is not in effect; -1 on error) */
int cuddh_ddh_set_march(void *ddh, int march);
int cuddh_ddh_march(void *ddh);
/* what the scaled march carries as the velocity: 0 auto, 1 q / (2 hm), 2 that times the head coefficient of the first sweep's
 * chain (cuddh_hip_ddh_plan_set_head); the getter returns the head in effect (1 or 2; 0 where march 2 is not in effect; -1 on error) */
int cuddh_ddh_set_head(void *ddh, int head);
int cuddh_ddh_head(void *ddh);
/* how head 2 forms the neighbour sums of its sweeps: 0 auto, 1 DPP on the vector pipe, 2 fetched both ways over the LDS pipe, the
 * same bits (cuddh_hip_ddh_plan_set_assembly); the getter returns the assembly in effect (1 or 2; 0 where head 2 is not in effect;
 * -1 on error) */
int cuddh_ddh_set_assembly(void *ddh, int assembly);
int cuddh_ddh_assembly(void *ddh);
/* the owner rule of kernels 11 and 12: last != 0 lets the last copy of every shared node publish instead of the first; same
 * results, a check (cuddh_hip_ddh_plan_set_owner_rule; an error on a plan that is neither kernel 11 nor kernel 12) */
int cuddh_ddh_set_owner_rule(void *ddh, int last);
/* traces are float for f64 == 0 and double otherwise */
int cuddh_ddh_rhs(void *ddh, const double *f, void *b);
int cuddh_ddh_postprocess(void *ddh, const void *lambda, const double *f, double *u);
int cuddh_ddh_action(void *ddh, const void *x, void *y);
int cuddh_ddh_local_traces(void *ddh, int d0, int d1, const double *f, const void *lambda, void *update);
/* the same for n listed subdomains (d_domains: DEVICE ints, distinct, in range) in one launch */
int cuddh_ddh_local_traces_listed(void *ddh, const int *d_domains, int n, const double *f, const void *lambda, void *update);
int cuddh_ddh_local_solution_listed(void *ddh, const int *d_domains, int n, const void *lambda, const double *f, double *u, int zero_u);
int cuddh_ddh_local_solution(void *ddh, int d0, int d1, const void *lambda, const double *f, double *u, int zero_u);
/* HOST copies of the constructor's tables: name in {"B","gI","sI"} (int) or
 * {"D","G","m","gmi","a","H","filter","cs","sn"} (float / double by f64).  count_only != 0: just return the length.
 * "filter", "cs" and "sn" are the base grid's; "filter@R", "cs@R", "sn@R" those of the grid of R times the mesh grid's steps,
 * for every R some subdomain marches on (cuddh_ddh_time_ratios); -1 + cuddh_last_error for any other R. */
long long cuddh_ddh_table(void *ddh, const char *name, void *h_out, int count_only);

/* ---- GMRES (reference include/gmres.hpp).  h_res / h_time: HOST arrays of maxit + 1 entries (may be NULL). */
typedef struct cuddh_solver_result
{
    int success;
    int num_iter;
    int num_matvec;
    int n_res; /* entries written to h_res / h_time */
} cuddh_solver_result;

int cuddh_gmres_f64(int n, double *x, void *op, const double *b, void *precond /* or NULL */, int m, int maxit, double tol,
                    int verbose, double max_seconds, cuddh_solver_result *out, double *h_res, double *h_time);
/* HelmholtzOperator::gmres: x, b in the reference ordering [u; v]; the iteration runs on plan-native vectors when the plan has them */
int cuddh_gmres_helmholtz(void *op, double *x, const double *b, int m, int maxit, double tol, int verbose, double max_seconds,
                          cuddh_solver_result *out, double *h_res, double *h_time);
/* op: a DDH handle (f64 == 0: float vectors, f64 != 0: double vectors) */
int cuddh_gmres_ddh(int n, void *x, void *ddh, const void *b, int m, int maxit, double tol, int verbose, double max_seconds,
                    cuddh_solver_result *out, double *h_res, double *h_time);
/* operator supplied by the caller: cb(ctx, x, y) must compute y = A x on DEVICE vectors on the library stream */
typedef void (*cuddh_action_cb)(void *ctx, const void *x, void *y);
int cuddh_gmres_callback(int n, void *x, cuddh_action_cb cb, void *ctx, const void *b, int is_f64, int m, int maxit, double tol,
                         int verbose, double max_seconds, cuddh_solver_result *out, double *h_res, double *h_time);
/* the same with vectors partitioned over processes (one per GPU): reduce(ctx, d_scalars, count, is_f64) must sum
 * `count` DEVICE scalars over all ranks in place, ordered on the library stream (an RCCL all-reduce) */
typedef void (*cuddh_reduce_cb)(void *ctx, void *d_scalars, int count, int is_f64);
int cuddh_gmres_callback_sharded(int n, void *x, cuddh_action_cb cb, void *ctx, cuddh_reduce_cb reduce, void *reduce_ctx,
                                 const void *b, int is_f64, int m, int maxit, double tol, int verbose, double max_seconds,
                                 cuddh_solver_result *out, double *h_res, double *h_time);

/* ---- the same five with the orthogonalisation of the Arnoldi step chosen: orth = 0 modified Gram-Schmidt (what the entry points
 * above do), 1 = classical Gram-Schmidt applied twice (CGS2: four launches per step whatever the step, three reductions of k + 1
 * scalars per step on the sharded path, orthogonality at working precision; m <= 512; csrc/include/cuddh/krylov.hpp).  Any other
 * value returns nonzero before anything touches the device, cuddh_last_error() beginning "gmres error: orthogonalization". */
int cuddh_gmres_f64_orth(int n, double *x, void *op, const double *b, void *precond /* or NULL */, int m, int maxit, double tol,
                         int verbose, double max_seconds, int orth, cuddh_solver_result *out, double *h_res, double *h_time);
int cuddh_gmres_helmholtz_orth(void *op, double *x, const double *b, int m, int maxit, double tol, int verbose, double max_seconds,
                               int orth, cuddh_solver_result *out, double *h_res, double *h_time);
int cuddh_gmres_ddh_orth(int n, void *x, void *ddh, const void *b, int m, int maxit, double tol, int verbose, double max_seconds,
                         int orth, cuddh_solver_result *out, double *h_res, double *h_time);
int cuddh_gmres_callback_orth(int n, void *x, cuddh_action_cb cb, void *ctx, const void *b, int is_f64, int m, int maxit, double tol,
                              int verbose, double max_seconds, int orth, cuddh_solver_result *out, double *h_res, double *h_time);
int cuddh_gmres_callback_sharded_orth(int n, void *x, cuddh_action_cb cb, void *ctx, cuddh_reduce_cb reduce, void *reduce_ctx,
                                      const void *b, int is_f64, int m, int maxit, double tol, int verbose, double max_seconds,
                                      int orth, cuddh_solver_result *out, double *h_res, double *h_time);

/* ---- the `_orth` five with `int augment` behind the orthogonalisation code: augment = k > 0 is LGMRES -- the last k corrections
 * x_i - x_{i-1} (normalised) and their images under the operator are kept and take the place of the last Krylov columns of every
 * cycle; their images are differences of residuals the iteration computes anyway, so no operator application is added and
 * num_matvec counts what was applied (csrc/include/cuddh/krylov.hpp: GmresOptions).  augment = 0 is the `_orth` entry point bit
 * for bit.  augment < 0 or >= m returns nonzero before anything touches the device, cuddh_last_error() beginning
 * "gmres error: augment". */
int cuddh_gmres_f64_aug(int n, double *x, void *op, const double *b, void *precond /* or NULL */, int m, int maxit, double tol,
                        int verbose, double max_seconds, int orth, int augment, cuddh_solver_result *out, double *h_res, double *h_time);
int cuddh_gmres_helmholtz_aug(void *op, double *x, const double *b, int m, int maxit, double tol, int verbose, double max_seconds,
                              int orth, int augment, cuddh_solver_result *out, double *h_res, double *h_time);
int cuddh_gmres_ddh_aug(int n, void *x, void *ddh, const void *b, int m, int maxit, double tol, int verbose, double max_seconds,
                        int orth, int augment, cuddh_solver_result *out, double *h_res, double *h_time);
int cuddh_gmres_callback_aug(int n, void *x, cuddh_action_cb cb, void *ctx, const void *b, int is_f64, int m, int maxit, double tol,
                             int verbose, double max_seconds, int orth, int augment, cuddh_solver_result *out, double *h_res, double *h_time);
int cuddh_gmres_callback_sharded_aug(int n, void *x, cuddh_action_cb cb, void *ctx, cuddh_reduce_cb reduce, void *reduce_ctx,
                                     const void *b, int is_f64, int m, int maxit, double tol, int verbose, double max_seconds,
                                     int orth, int augment, cuddh_solver_result *out, double *h_res, double *h_time);
/* The same iteration over the COMPLEX numbers (GmresOptions::arithmetic = complex, csrc/include/cuddh/krylov.hpp): x and b hold
 * n / 2 complex numbers, real parts in the first half and imaginary parts in the second (a DDH trace vector [lambda; mu]), the operator
 * must be complex-linear in that sense (to a few 1e-3 is enough: the true residual ends every cycle and decides), and m operator
 * applications minimise over complex instead of real combinations of the Krylov vectors with the same vectors, bytes and launches.
 * Modified Gram-Schmidt, no augmentation, single process; argument lists of cuddh_gmres_ddh / cuddh_gmres_callback.  An odd n or
 * m outside [1, 512] returns nonzero, cuddh_last_error() beginning "gmres error: complex arithmetic". */
int cuddh_gmres_ddh_cplx(int n, void *x, void *ddh, const void *b, int m, int maxit, double tol, int verbose, double max_seconds,
                         cuddh_solver_result *out, double *h_res, double *h_time);
int cuddh_gmres_callback_cplx(int n, void *x, cuddh_action_cb cb, void *ctx, const void *b, int is_f64, int m, int maxit, double tol,
                              int verbose, double max_seconds, cuddh_solver_result *out, double *h_res, double *h_time);
/* The small problem of one GMRES(m) cycle on HOST arrays, as the solvers above run it (Givens rotations of the Hessenberg columns,
 * residual estimate, back substitution); no GPU.  h_cols: ncols columns one after another, column k as k + 2 entries h_0 .. h_k and
 * the norm h_{k+1}; entries are double (is_f64), float (neither flag) or re, im pairs of doubles (is_complex, whatever is_f64).
 * beta: |r| at the start of the cycle.  y_out: the ncols coefficients in the entries' format; est_out: the ncols residual estimates
 * after each column, double.  m < 1, ncols outside [1, m] or a null pointer returns nonzero and writes nothing. */
int cuddh_gmres_small_problem(int is_complex, int is_f64, int m, int ncols, const void *h_cols, double beta, void *y_out, double *est_out);

/* ---- whole-domain WaveHoltz (csrc/include/cuddh/waveholtz.hpp): the filtered time-domain iteration for
 * (K - w^2 M + i w H) U = f on the whole space, M = diag(a^2 m) and H = diag(a h) lumped.  The handle is an OPERATOR handle of
 * size 2 ndof whose action is y = x - S x: cuddh_operator_apply, cuddh_operator_apply_add, cuddh_operator_destroy and
 * cuddh_gmres_f64 (and its _orth / _aug forms) take it.  h_a: HOST nodal coefficient (ndof), finite and positive.
 * integrator 0 = RK2 (coarsen must be 1), 1 = RK4 on ceil(nt_mesh / coarsen) steps, coarsen in [1, 16]; time_ratio in [1, 256]
 * multiplies the step count, 0 = from the coefficient, max(1, ceil((1 - 1e-9) / min a)); stiffness 0 = the Gauss-Legendre rule of
 * cuddh_stiffness_create(fem, 0), 1 = the n_basis-point Gauss-Lobatto rule (the collocated stiffness of the DDH local solves);
 * h_faces HOST edge ids of the absorbing faces, n_faces < 0 = every boundary edge.  Anything else is refused before anything is
 * allocated (NULL + cuddh_last_error, the message starts with "WaveHoltz error"). */
void *cuddh_waveholtz_create(double omega, const double *h_a, void *fem, int integrator, int coarsen, int time_ratio, int stiffness,
                             const int *h_faces, int n_faces);
/* z_out = W(z_in; f) (DEVICE, 2 ndof each): one filtered period from z_in (NULL: from zero) under the load f = [f_re; f_im]
 * (NULL: none).  The right-hand side of (I - S) z = b is b = W(0; f). */
int cuddh_waveholtz_period(void *op, const double *z_in, const double *f, double *z_out);
/* u = [z_u; z_v / omega], real and imaginary part of U (DEVICE, 2 ndof; u may be z) */
int cuddh_waveholtz_solution(void *op, const double *z, double *u);
/* h_info = {nt, time ratio, integrator, coarsen, sweeps per period, ndof}; *h_dt = time step; kernel (cap bytes, may be NULL):
 * the kernel of the stiffness sweep, "generic" before the first period.  Returns 0, nonzero on error. */
int cuddh_waveholtz_info(void *op, int *h_info, double *h_dt, char *kernel, int cap);
/* cuddh_waveholtz_create with the form of the sweep behind its arguments: 0 = a stiffness apply and a stage kernel per sweep (what
 * cuddh_waveholtz_create builds), 1 = lattice: one launch per sweep does the stiffness stencil and the stage on lattice-ordered
 * vectors (cuddh_hip_wave_lattice_*).  The lattice form needs stiffness = 1 and a uniform rectangle mesh, which is
 * detected (cuddh_wave_lattice_map); anything else is refused before anything is allocated, the message starts with
 * "WaveHoltz error: sweep:".  Every entry point above takes the handle unchanged: z, f and u keep the space's dof order.  In
 * that form cuddh_waveholtz_info's kernel is "wave_lattice nb<n_basis>". */
void *cuddh_waveholtz_create_sweep(double omega, const double *h_a, void *fem, int integrator, int coarsen, int time_ratio, int stiffness,
                                   const int *h_faces, int n_faces, int sweep);
/* the form of the sweep: 0 or 1 as above, -1 when op is not a WaveHoltz handle */
int cuddh_waveholtz_sweep(void *op);
/* cuddh_waveholtz_create_sweep with the precision of the march behind its arguments: 0 = f64 (what the two entry points above
 * build), 1 = f32: the lattice form with its thirteen lattice vectors stored and its sweeps computed in fp32
 * (cuddh_hip_wave32_*), half the march's memory.  z, f, b and u stay fp64 in the space's dof order; they are rounded
 * once on the way into a period and converted once on the way out, and y = x - S x is formed in double.  The option is for
 * tolerances around 1e-4: the fp32 operator's own defect is about 1e-6.  Any other value, or 1 with sweep = 0, is refused before
 * anything is allocated (NULL, the message starts with "WaveHoltz error: precision:").  In that form cuddh_waveholtz_info's
 * kernel is "wave_lattice nb<n_basis> f32". */
void *cuddh_waveholtz_create_precision(double omega, const double *h_a, void *fem, int integrator, int coarsen, int time_ratio, int stiffness,
                                       const int *h_faces, int n_faces, int sweep, int precision);
/* the precision of the march: 0 or 1 as above, -1 when op is not a WaveHoltz handle */
int cuddh_waveholtz_precision(void *op);
/* cuddh_waveholtz_create_precision with the launches of the lattice march behind its arguments: 0 = one launch per sweep (what the
 * entry points above build), 1 = one launch per pair of sweeps (cuddh_hip_wave_pair_*, cuddh_hip_wave_pair32_*):
 * rk2_a with rk2_b, rk4_1 with rk4_2, rk4_3 with rk4_4, in either precision.  The march is the per-sweep one bit for bit, in half
 * the launches.  Any other value, or 1 without sweep = 1, is refused before anything is allocated (NULL, the message starts with
 * "WaveHoltz error: launch:").  In that form cuddh_waveholtz_info's kernel is "wave_pair nb<n_basis>" ("... f32"). */
void *cuddh_waveholtz_create_launch(double omega, const double *h_a, void *fem, int integrator, int coarsen, int time_ratio, int stiffness,
                                    const int *h_faces, int n_faces, int sweep, int precision, int launch);
/* the launches of the march: 0 or 1 as above, -1 when op is not a WaveHoltz handle */
int cuddh_waveholtz_launch(void *op);
/* The lattice behind a space on a uniform rectangle mesh (csrc/include/cuddh/wave_lattice.hpp; host code, no device is touched):
 * h_dims = {nx, ny, Lx, Ly, stride}, L = n (n_basis - 1) + 1 nodes per direction and stride = Lx rounded up to even, the doubles
 * per row of the lattice vectors; h_h = {hx, hy}; h_node_of (ndof): dof -> I + Lx J.  Each may be NULL.  The mesh qualifies when
 * its elements are axis-aligned rectangles, congruent to 1e-12 of their size, with element e at (e % nx, e / nx); the map is
 * verified to be a bijection that agrees on shared nodes and with the collocation points.  Returns 0, or nonzero with
 * cuddh_last_error() beginning "WaveHoltz error: sweep:". */
int cuddh_wave_lattice_map(void *fem, int *h_dims, double *h_h, int *h_node_of);
/* The lattice behind a space on a grid mesh with missing cells (host code): the elements are a subset of the cells of
 * a uniform nx x ny grid, listed in ascending cell index i + nx j with cuddh_mesh_uniform_rect's corner order (what
 * cuddh_mesh_grid_cells builds; a full grid qualifies too).  hx, hy come from element 0, the origin and nx, ny from the bounding
 * box of all corners, an element's cell from its first corner.  h_dims, h_h as above; h_node_of (ndof): dof -> I + Lx J, an
 * injection whose image is the nodes of the existing cells; h_cell (nx * ny bytes): 1 where cell i + nx j exists.  Each may be
 * NULL.  Verified: every corner is where its cell has it (the tolerance above), cell indices strictly increase, shared nodes
 * agree and match the collocation points, the map is injective, Lx Ly and stride Ly fit in an int.  Returns 0, or nonzero with
 * cuddh_last_error() beginning "WaveHoltz error: sweep:" and nothing written.  cuddh_waveholtz_create_sweep and its successors try
 * cuddh_wave_lattice_map first and this detection where that refuses; a mesh with missing cells runs cuddh_hip_wave_cells_*
 * (kernel "wave_cells nb<n_basis>", "... f32"), and launch = 1 on it is refused ("WaveHoltz error: launch:"). */
int cuddh_wave_lattice_map_cells(void *fem, int *h_dims, double *h_h, int *h_node_of, unsigned char *h_cell);
/* cuddh_waveholtz_create_launch with a per-cell stiffness coefficient behind its arguments: h_beta, HOST, one value
 * per element in element order, each finite and positive.  The problem is  -div(beta grad U) - w^2 a^2 U = f  with beta constant
 * on each element; the march runs cuddh_hip_wave_weights_* / cuddh_hip_wave_weights32_* (cuddh_waveholtz_info's kernel is
 * "wave_weights nb<n_basis>", "... f32") on a full rectangle and on a grid with missing cells alike.  Refused before anything is
 * allocated (NULL): a NULL h_beta, a value that is not finite and positive, sweep != 1 ("WaveHoltz error: cell_stiffness:");
 * launch = 1 ("WaveHoltz error: launch:": there is no paired form).  time_ratio = 0 is cuddh_waveholtz_coefficient_ratio's rule.
 * Mass and faces are unchanged (M = diag(a^2 m), H = diag(a h)): the absorbing faces discretise  beta dU/dn + i w a U = 0,  the
 * first-order absorbing condition only where beta = 1 along them. */
void *cuddh_waveholtz_create_cell_stiffness(double omega, const double *h_a, void *fem, int integrator, int coarsen, int time_ratio, int stiffness,
                                            const int *h_faces, int n_faces, int sweep, int precision, int launch, const double *h_beta);
/* Plain host code.  The cell weights the weighted kernels read: h_beta as above on the cell grid the lattice detection finds for
 * fem (cuddh_wave_lattice_map, and where that refuses cuddh_wave_lattice_map_cells).  On a full rectangle element e is cell e; on
 * a grid with missing cells the present cells in ascending order take the values in element order and absent cells get 0.
 * h_weights (nx * ny, cell (a, b) at a + nx b) and h_dims (2: nx, ny) may each be NULL.  Returns 0, or nonzero with
 * cuddh_last_error() beginning "WaveHoltz error: cell_stiffness:" or "WaveHoltz error: sweep:" and nothing written. */
int cuddh_wave_lattice_cell_weights(void *fem, const double *h_beta, double *h_weights, int *h_dims);
/* Plain host code.  The ratio time_ratio = 0 chooses: max(1, ceil((1 - 1e-9) max_e (sqrt(beta_e) / min_{g in e} a_g))), the local
 * wave speed being sqrt(beta) / a.  h_I (nodes_per_elem x n_elem): element node -> dof; h_a the nodal coefficient; h_beta n_elem
 * values or NULL (beta == 1: the rule of cuddh_waveholtz_create).  Returns 0 and the ratio in *h_ratio, or nonzero with
 * cuddh_last_error() beginning "WaveHoltz error: time step:" (above 256) or "WaveHoltz error: cell_stiffness:" and nothing written. */
int cuddh_waveholtz_coefficient_ratio(int n_elem, int nodes_per_elem, const int *h_I, const double *h_a, const double *h_beta, int *h_ratio);
/* the 1-D tables of the lattice form on the reference element: h_A (n_basis x n_basis, row-major) = D^T diag(w) D, h_w (n_basis) */
int cuddh_wave_lattice_tables(void *basis, double *h_A, double *h_w);

/* ---- whole-domain WaveHoltz in three dimensions (csrc/include/cuddh/waveholtz_box.hpp): the iteration above on a
 * box [ax, bx] x [ay, by] x [az, bz] of nx x ny x nz congruent brick elements with n_basis in [2, 8] Gauss-Lobatto points per
 * direction, on the kernels cuddh_hip_wave_box_* (cuddh_hip.h states the operators K, m, h and the layout).  h_box = {ax, bx, ay,
 * by, az, bz}; h_a: HOST coefficient, one finite positive value per lattice node, node (I, J, K) at I + Lx (J + Ly K), L = n
 * (n_basis - 1) + 1; integrator, coarsen and time_ratio as for cuddh_waveholtz_create, the mesh size being min(hx, hy, hz);
 * face_mask: bits 0..5 = the faces x = ax, x = bx, y = ay, y = by, z = az, z = bz absorbing, the others sound-hard.  The handle
 * is an OPERATOR handle of size 2 Lx Ly Lz whose action is y = x - S x, exactly like cuddh_waveholtz_create's; vectors are in the
 * lattice order above.  Anything else is refused before anything is allocated (NULL + cuddh_last_error; the message starts with
 * "WaveHoltz error: box:", "WaveHoltz error: time step:" or "WaveHoltz error: integrator:"). */
void *cuddh_waveholtz_box_create(double omega, int nx, int ny, int nz, const double *h_box, int n_basis, const double *h_a, int integrator,
                                 int coarsen, int time_ratio, int face_mask);
/* Plain host code, nothing is allocated: every refusal of cuddh_waveholtz_box_create, then the period's grid such an operator
 * marches on: h_steps = {nt, the time ratio in effect}, nt = ratio * ceil(mesh_grid_steps(omega, min(hx, hy, hz), n_basis) /
 * coarsen), and *h_dt = 2 pi / (omega nt).  Returns 0, or nonzero with cuddh_last_error() as above and nothing written. */
int cuddh_waveholtz_box_time_grid(double omega, int nx, int ny, int nz, const double *h_box, int n_basis, const double *h_a, int integrator,
                                  int coarsen, int time_ratio, int face_mask, int *h_steps, double *h_dt);
/* cuddh_waveholtz_period, _solution and _info for such a handle; the kernel is "wave_box nb<n_basis>", followed by
 * " (run-time n_basis)" where n_basis is no compile-time form; h_info[5] = Lx Ly Lz */
int cuddh_waveholtz_box_period(void *op, const double *z_in, const double *f, double *z_out);
int cuddh_waveholtz_box_solution(void *op, const double *z, double *u);
int cuddh_waveholtz_box_info(void *op, int *h_info, double *h_dt, char *kernel, int cap);
/* h_dims = {Lx, Ly, Lz} */
int cuddh_waveholtz_box_lattice(void *op, int *h_dims);
/* cuddh_waveholtz_box_create with the precision of the march: 0 = f64, which is cuddh_waveholtz_box_create itself,
 * 1 = f32: the lattice vectors, the stencil and the stages in fp32 on the kernels cuddh_hip_wave_box32_*, rows of the padded lattice
 * a multiple of four floats; z_in, f, invm and Hi are rounded to float once on the way in, every vector of this interface, the
 * action y = x - S x and the solution stay double.  The period's grid does not depend on it.  fp32 suits GMRES tolerances around
 * 1e-4, not 1e-6.  The kernel is then "wave_box nb<n_basis> f32", followed by " (run-time n_basis)" for n_basis other than 4 and 5.
 * Any other code is refused like the rest (NULL, "WaveHoltz error: precision:"). */
void *cuddh_waveholtz_box_create_precision(double omega, int nx, int ny, int nz, const double *h_box, int n_basis, const double *h_a,
                                           int integrator, int coarsen, int time_ratio, int face_mask, int precision);
/* 0 (f64) or 1 (f32); -1 with cuddh_last_error() for a handle that is no such operator */
int cuddh_waveholtz_box_precision(void *op);

#ifdef __cplusplus
}
#endif
#endif /* CUDDH_CAPI_H */
