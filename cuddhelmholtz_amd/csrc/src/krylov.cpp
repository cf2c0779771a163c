// Restarted GMRES.  Iteration semantics follow reference source/gmres.cpp:91-235
// (see krylov.hpp); the arithmetic is scheduled differently: the k+1 projection
// coefficients of an Arnoldi step stay on the device (each axpy reads its
// coefficient from device memory) and reach the host in one copy per step.
#include "cuddh/krylov.hpp"

#include <algorithm>
#include <cmath>
#include <complex>
#include <string>

#include "cuddh_hip.h"

namespace cuddh
{
    namespace
    {
        // ---- scalar-type dispatch onto the C ABI
        inline int k_dot(int n, const double *x, const double *y, double *r, void *ws) { return cuddh_hip_dot_f64(n, x, y, r, ws, stream()); }
        inline int k_dot(int n, const float *x, const float *y, float *r, void *ws) { return cuddh_hip_dot_f32(n, x, y, r, ws, stream()); }
        inline int k_axpby_dev(int n, double sa, const double *a, const double *x, double b, double *y) { return cuddh_hip_axpby_dev_f64(n, sa, a, x, b, y, stream()); }
        inline int k_axpby_dev(int n, float sa, const float *a, const float *x, float b, float *y) { return cuddh_hip_axpby_dev_f32(n, sa, a, x, b, y, stream()); }
        inline int k_mgs_stage(int n, double *w, const double *vp, const double *vn, const double *pi, double *po, double *h) { return cuddh_hip_mgs_stage_f64(n, w, vp, vn, pi, po, h, stream()); }
        inline int k_mgs_stage(int n, float *w, const float *vp, const float *vn, const float *pi, float *po, float *h) { return cuddh_hip_mgs_stage_f32(n, w, vp, vn, pi, po, h, stream()); }
        inline int k_mgs_finish(int n, double *w, const double *pi, double *h) { return cuddh_hip_mgs_finish_f64(n, w, pi, h, stream()); }
        inline int k_mgs_finish(int n, float *w, const float *pi, float *h) { return cuddh_hip_mgs_finish_f32(n, w, pi, h, stream()); }
        inline int k_cgs_pass(int n, double *w, const double *V, long long ldv, int k1, int update, int dots, const double *cin, int ncin, long long cstride,
                              const double *hacc, double *hout, double *pout)
        {
            return cuddh_hip_cgs_pass_f64(n, w, V, ldv, k1, update, dots, cin, ncin, cstride, hacc, hout, pout, stream());
        }
        inline int k_cgs_pass(int n, float *w, const float *V, long long ldv, int k1, int update, int dots, const float *cin, int ncin, long long cstride,
                              const float *hacc, float *hout, float *pout)
        {
            return cuddh_hip_cgs_pass_f32(n, w, V, ldv, k1, update, dots, cin, ncin, cstride, hacc, hout, pout, stream());
        }
        inline int k_cgs_reduce(int n, int k1, const double *p, double *out) { return cuddh_hip_cgs_reduce_f64(n, k1, p, out, stream()); }
        inline int k_cgs_reduce(int n, int k1, const float *p, float *out) { return cuddh_hip_cgs_reduce_f32(n, k1, p, out, stream()); }
        inline int k_update(int n, double *x, double *dx, const double *V, long long ldv, int nv, const double *Z, long long ldz, int nz, const double *coef, double *pout)
        {
            return cuddh_hip_krylov_update_f64(n, x, dx, V, ldv, nv, Z, ldz, nz, coef, pout, stream());
        }
        inline int k_update(int n, float *x, float *dx, const float *V, long long ldv, int nv, const float *Z, long long ldz, int nz, const float *coef, float *pout)
        {
            return cuddh_hip_krylov_update_f32(n, x, dx, V, ldv, nv, Z, ldz, nz, coef, pout, stream());
        }

        inline int k_cmgs_stage(int h, double *w, const double *vp, const double *vn, const double *pi, double *po, double *c) { return cuddh_hip_cmgs_stage_f64(h, w, vp, vn, pi, po, c, stream()); }
        inline int k_cmgs_stage(int h, float *w, const float *vp, const float *vn, const float *pi, float *po, float *c) { return cuddh_hip_cmgs_stage_f32(h, w, vp, vn, pi, po, c, stream()); }
        inline int k_cupdate(int h, double *x, const double *V, long long ldv, int k1, const double *coef) { return cuddh_hip_ckrylov_update_f64(h, x, V, ldv, k1, coef, stream()); }
        inline int k_cupdate(int h, float *x, const float *V, long long ldv, int k1, const float *coef) { return cuddh_hip_ckrylov_update_f32(h, x, V, ldv, k1, coef, stream()); }

        // apply the k previous rotations to column h, then build rotation k that zeroes h[k+1]
        template <typename scalar>
        void rotate_column(scalar *h, scalar *cs, scalar *sn, int k)
        {
            for (int i = 0; i < k; ++i)
            {
                const scalar a = h[i], b = h[i + 1];
                h[i] = cs[i] * a + sn[i] * b;
                h[i + 1] = cs[i] * b - sn[i] * a;
            }
            const scalar r = std::hypot(h[k], h[k + 1]);
            cs[k] = h[k] / r;
            sn[k] = h[k + 1] / r;
            h[k] = cs[k] * h[k] + sn[k] * h[k + 1];
            h[k + 1] = 0;
        }

        // back substitution R y = g for the leading kk x kk block of the (ld x m) column-major array R
        // (the reference calls LAPACK ?trsv('U','N','N'), source/gmres.cpp:26-41)
        template <typename scalar>
        void back_substitute(int kk, const scalar *R, int ld, scalar *g)
        {
            for (int i = kk - 1; i >= 0; --i)
            {
                scalar s = g[i];
                for (int j = i + 1; j < kk; ++j)
                    s -= R[i + ld * j] * g[j];
                g[i] = s / R[i + ld * i];
            }
        }

        class LeftPreconditioned : public Operator
        {
        public:
            LeftPreconditioned(int n, const Operator *A_, const Operator *P_) : tmp(n), A(A_), P(P_) {}

            void action(double, const double *, double *) const override
            {
                cuddh_error("gmres: the preconditioned system only supports action(x, y).");
            }

            void action(const double *x, double *y) const override
            {
                double *q = tmp.device_write();
                A->action(x, q);
                P->action(q, y);
            }

        private:
            mutable host_device_dvec tmp;
            const Operator *A;
            const Operator *P;
        };

        template <typename scalar, typename Op>
        solver_out arnoldi_restarted(int n, scalar *x, const Op *A, const scalar *b, int m, int maxit, scalar tol, int verbose,
                                     double max_seconds, const ScalarReduce *red = nullptr, Orthogonalization orth = Orthogonalization::mgs, int augment = 0)
        {
            using clock = std::chrono::high_resolution_clock;
            const scalar one = 1, zero = 0;
            const int m1 = m + 1;
            constexpr int is_f64 = sizeof(scalar) == 8;

            const bool cgs2 = orth == Orthogonalization::cgs2;
            if (orth != Orthogonalization::mgs && !cgs2)
                cuddh_error("gmres error: orthogonalization must be mgs or cgs2.");
            if (cgs2 && m > 512)
                cuddh_error("gmres error: orthogonalization cgs2 takes restart lengths up to 512 (one launch covers the whole basis).");
            // augment = k > 0 (LGMRES, krylov.hpp): the last k corrections z and their images A z take the place of the last Krylov columns
            if (augment < 0 || (augment > 0 && augment >= m))
                cuddh_error("gmres error: augment must be in [0, m - 1].");
            if (augment > 0 && m > 512)
                cuddh_error("gmres error: augment takes restart lengths up to 512 (one launch of the update covers every column).");
            // distance of two basis vectors: n; under cgs2 and with augment > 0 rounded up to 16 bytes, so that one launch may read all of
            // them as 16-byte vectors
            constexpr std::size_t per16 = 16 / sizeof(scalar);
            const std::size_t ldv = (cgs2 || augment > 0) ? (static_cast<std::size_t>(n) + per16 - 1) / per16 * per16 : static_cast<std::size_t>(n);

            HostDeviceArray<scalar> r_store(n), V_store(ldv * m1), col_store(m1 + 1);
            scalar *r = r_store.device_write();
            scalar *V = V_store.device_write();
            scalar *dcol = col_store.device_write(); // Hessenberg column under construction, on the device

            void *ws = nullptr;
            detail::check_hip(cuddh_hip_malloc_zeroed(&ws, cuddh_hip_reduce_ws_bytes()), "gmres workspace");
            struct Guard
            {
                void *p;
                ~Guard() { cuddh_hip_free(p); }
            } guard{ws};

            // cgs2: two partial-sum buffers (cuddh_hip.h: rows of `row` scalars, <w, w> in row 0), the first pass's coefficients, and for
            // partitioned vectors the second pass's reduced coefficients and a row that holds the reduced <w, w> followed by zeros
            // (a pass and cgs_reduce do nothing on an empty vector, so a rank without entries would send stale coefficients into the sums)
            if (cgs2 && red && n == 0)
                cuddh_error("gmres error: orthogonalization cgs2 needs at least one entry of the partitioned vectors on every rank.");
            void *cgs_ws = nullptr;
            std::size_t row = 0;
            scalar *pA = nullptr, *pB = nullptr, *dc1 = nullptr, *dc2 = nullptr, *zrow = nullptr;
            int n_part = 0;
            if (cgs2)
            {
                row = cuddh_hip_cgs_ws_bytes(0) / sizeof(double);
                const std::size_t pbytes = cuddh_hip_cgs_ws_bytes(m);
                detail::check_hip(cuddh_hip_malloc_zeroed(&cgs_ws, 2 * pbytes + (2 * (m1 + 1) + row) * sizeof(double)), "gmres cgs2 workspace");
                pA = static_cast<scalar *>(cgs_ws);
                pB = reinterpret_cast<scalar *>(static_cast<char *>(cgs_ws) + pbytes);
                dc1 = reinterpret_cast<scalar *>(static_cast<char *>(cgs_ws) + 2 * pbytes);
                dc2 = dc1 + (m1 + 1);
                zrow = dc2 + (m1 + 1);
                n_part = cuddh_hip_cgs_partials(n);
            }
            Guard cgs_guard{cgs_ws};

            // augment: the pairs (z_p, A z_p), most recent first, ldv apart like the basis; the correction of a cycle; on the device the
            // coefficients of the update, a row of partial sums of |dx|^2 (the <w, w> row of a cgs pass) and their sum
            HostDeviceArray<scalar> Z_store, AZ_store, dx_store;
            scalar *Zs = nullptr, *AZs = nullptr, *dxv = nullptr, *d_part = nullptr, *d_coef = nullptr, *d_dxx = nullptr;
            void *aug_ws = nullptr;
            if (augment > 0)
            {
                Z_store.resize(static_cast<int>(ldv * augment));
                AZ_store.resize(static_cast<int>(ldv * augment));
                dx_store.resize(n);
                Zs = Z_store.device_write();
                AZs = AZ_store.device_write();
                dxv = dx_store.device_write();
                const std::size_t prow = cuddh_hip_cgs_ws_bytes(0);
                detail::check_hip(cuddh_hip_malloc_zeroed(&aug_ws, prow + (m + 1) * sizeof(double)), "gmres augmentation workspace");
                d_part = static_cast<scalar *>(aug_ws);
                d_coef = reinterpret_cast<scalar *>(static_cast<char *>(aug_ws) + prow);
                d_dxx = d_coef + m;
            }
            Guard aug_guard{aug_ws};
            int n_pairs = 0;

            // Operators that only queue device work (operator.hpp: QueuesDeviceWorkOnly) are driven one Arnoldi step ahead of the host:
            // two pinned Hessenberg columns and two events
            const bool ahead = !red && dynamic_cast<const QueuesDeviceWorkOnly *>(A) != nullptr;
            struct AheadBuffers
            {
                scalar *pin[2] = {nullptr, nullptr};
                void *ev[2] = {nullptr, nullptr};
                ~AheadBuffers()
                {
                    for (int i = 0; i < 2; ++i)
                    {
                        (void)cuddh_hip_host_free(pin[i]);
                        (void)cuddh_hip_event_destroy(ev[i]);
                    }
                }
            } ab;
            if (ahead)
                for (int i = 0; i < 2; ++i)
                {
                    detail::check_hip(cuddh_hip_host_alloc(reinterpret_cast<void **>(&ab.pin[i]), sizeof(scalar) * (m1 + 1)), "gmres pinned column");
                    detail::check_hip(cuddh_hip_event_create(&ab.ev[i]), "gmres event");
                }
            scalar *const *pin = ab.pin;
            void *const *ev = ab.ev;

            // 2-norm; with partitioned vectors the sum of squares is reduced over the ranks first
            auto norm_of = [&](const scalar *v) -> scalar
            {
                if (!red)
                    return norm(n, v);
                scalar ss = 0;
                detail::check_hip(k_dot(n, v, v, dcol, ws), "gmres norm");
                red->fn(red->user, dcol, 1, is_f64);
                detail::check_hip(cuddh_hip_stream_sync(stream()), "gmres sync");
                detail::check_hip(cuddh_hip_copy_d2h_on(&ss, dcol, sizeof(scalar), stream()), "gmres norm copy");
                return std::sqrt(ss);
            };

            const scalar bnrm = norm_of(b);

            std::vector<scalar> H(static_cast<std::size_t>(m1) * m, 0), cs(m, 0), sn(m, 0), eta(m1, 0);

            solver_out out;
            out.success = false;
            out.num_iter = 0;
            out.num_matvec = 0;
            out.res_norm.reserve(maxit + 1);
            out.time.reserve(maxit + 1);

            A->action(x, r);
            out.num_matvec++;
            axpby(n, one, b, -one, r); // r = b - A x
            scalar r_nrm = norm_of(r);

            out.res_norm.push_back(static_cast<double>(r_nrm));
            out.time.push_back(0.0);
            const auto t0 = clock::now();

            if (r_nrm < tol * bnrm)
            {
                out.success = true;
                if (verbose)
                    std::cout << "After 0 iterations, GMRES achieved rel. residual of " << out.res_norm.back() / bnrm
                              << "\nGMRES successfully converged within desired tolerance." << std::endl;
                return out;
            }

            if (verbose)
                std::cout << std::setprecision(5) << std::scientific;

            int it = 1;
            for (; it < maxit; ++it)
            {
                axpby(n, one / r_nrm, r, zero, V); // v0 = r / ||r||
                // columns k < n_krylov are Krylov columns (w = A v_k); column n_krylov + p takes w = A z_p from the stored pair: a copy,
                // no operator application (augment = 0: n_krylov = m)
                const int n_krylov = m - std::min(augment, n_pairs);
                auto next_w = [&](int k, const scalar *vk, scalar *vk1)
                {
                    if (k < n_krylov)
                        A->action(vk, vk1);
                    else
                        copy(n, AZs + static_cast<std::size_t>(k - n_krylov) * ldv, vk1);
                };
                std::fill(eta.begin(), eta.end(), zero);
                eta[0] = r_nrm;

                // One Arnoldi step queued on the stream: w = A v_k, modified Gram-Schmidt against v_0..v_k as a chain of fused stages
                // (stage j applies the projection on v_{j-1} and leaves the partial sums of <w, v_j> -- the last one <w, w> -- for
                // the next stage, so one launch per basis vector does what dot + reduce + axpy did; coefficients stay on the device),
                // normalisation.  On breakdown (norm == 0) v_{k+1} becomes non-finite but is never used.
                // cgs2: classical Gram-Schmidt against all of v_0..v_k at once, twice -- pass A the k + 1 inner products, pass B the
                // projection with their sums and the inner products of the result, pass C the projection with those (h_j = c1_j + c2_j)
                // and <w, w>, then the same normalisation: four launches at every k
                auto queue_step_cgs2 = [&](int k, scalar *vk1)
                {
                    const int k1 = k + 1;
                    const scalar *none = nullptr;
                    detail::check_hip(k_cgs_pass(n, vk1, V, ldv, k1, 0, 1, none, 0, 0, none, static_cast<scalar *>(nullptr), pA), "gmres cgs2 pass");
                    detail::check_hip(k_cgs_pass(n, vk1, V, ldv, k1, 1, 1, pA + row, n_part, row, none, dc1, pB), "gmres cgs2 pass");
                    detail::check_hip(k_cgs_pass(n, vk1, V, ldv, k1, 1, 2, pB + row, n_part, row, dc1, dcol, pA), "gmres cgs2 pass");
                    detail::check_hip(k_mgs_finish(n, vk1, pA, dcol + k1), "gmres normalise");
                };

                auto queue_step = [&](int k)
                {
                    scalar *vk = V + static_cast<std::size_t>(k) * ldv;
                    scalar *vk1 = vk + ldv;
                    next_w(k, vk, vk1);
                    if (cgs2)
                        queue_step_cgs2(k, vk1);
                    else
                    {
                        scalar *pa = static_cast<scalar *>(ws), *pb = pa + cuddh_hip_reduce_ws_bytes() / (2 * sizeof(double));
                        detail::check_hip(k_mgs_stage(n, vk1, static_cast<const scalar *>(nullptr), V, pa, pa, dcol), "gmres mgs");
                        for (int j = 0; j <= k; ++j)
                        {
                            const scalar *vj = V + static_cast<std::size_t>(j) * ldv;
                            const scalar *vnext = (j < k) ? vj + ldv : nullptr;
                            detail::check_hip(k_mgs_stage(n, vk1, vj, vnext, pa, pb, dcol + j), "gmres mgs");
                            std::swap(pa, pb);
                        }
                        detail::check_hip(k_mgs_finish(n, vk1, pa, dcol + k + 1), "gmres normalise");
                    }
                    if (ahead)
                    {
                        // the Hessenberg column leaves for pinned host memory behind the step; the next step may be queued behind it
                        detail::check_hip(cuddh_hip_copy_d2h_async(pin[k & 1], dcol, sizeof(scalar) * (k + 2), stream()), "gmres column copy");
                        detail::check_hip(cuddh_hip_event_record(ev[k & 1], stream()), "gmres event");
                    }
                };

                int k1 = 0;
                if (ahead)
                    queue_step(0);
                for (int k = 0; k < m; ++k)
                {
                    k1 = k + 1;
                    scalar *vk = V + static_cast<std::size_t>(k) * ldv;
                    scalar *vk1 = vk + ldv;
                    scalar *h = H.data() + static_cast<std::size_t>(m1) * k;

                    if (red && cgs2)
                    {
                        // partitioned vectors: the k + 1 sums of a pass are reduced over the ranks in one call, and the next pass reads
                        // the reduced coefficients (ncin = 1); three reductions per step
                        next_w(k, vk, vk1);
                        const scalar *none = nullptr;
                        detail::check_hip(k_cgs_pass(n, vk1, V, ldv, k1, 0, 1, none, 0, 0, none, static_cast<scalar *>(nullptr), pA), "gmres cgs2 pass");
                        detail::check_hip(k_cgs_reduce(n, k1, pA, dcol), "gmres cgs2 reduce");
                        red->fn(red->user, dcol, k1, is_f64);
                        detail::check_hip(k_cgs_pass(n, vk1, V, ldv, k1, 1, 1, dcol, 1, 1, none, dc1, pB), "gmres cgs2 pass");
                        detail::check_hip(k_cgs_reduce(n, k1, pB, dc2), "gmres cgs2 reduce");
                        red->fn(red->user, dc2, k1, is_f64);
                        detail::check_hip(k_cgs_pass(n, vk1, V, ldv, k1, 1, 2, dc2, 1, 1, dc1, dcol, pA), "gmres cgs2 pass");
                        detail::check_hip(k_cgs_reduce(n, 0, pA, zrow), "gmres cgs2 reduce"); // zrow[0] = <w, w> of this rank; zeros behind it
                        red->fn(red->user, zrow, 1, is_f64);
                        detail::check_hip(k_mgs_finish(n, vk1, zrow, dcol + k1), "gmres normalise");
                        detail::check_hip(cuddh_hip_stream_sync(stream()), "gmres sync");
                        detail::check_hip(cuddh_hip_copy_d2h_on(h, dcol, sizeof(scalar) * (k1 + 1), stream()), "gmres column copy");
                    }
                    else if (red)
                    {
                        next_w(k, vk, vk1);
                        // partitioned vectors: every coefficient is summed over the ranks before it is applied
                        for (int j = 0; j < k1; ++j)
                        {
                            const scalar *vj = V + static_cast<std::size_t>(j) * ldv;
                            detail::check_hip(k_dot(n, vk1, vj, dcol + j, ws), "gmres dot");
                            red->fn(red->user, dcol + j, 1, is_f64);
                            detail::check_hip(k_axpby_dev(n, -one, dcol + j, vj, one, vk1), "gmres projection");
                        }
                        detail::check_hip(k_dot(n, vk1, vk1, dcol + k1, ws), "gmres dot");
                        red->fn(red->user, dcol + k1, 1, is_f64);
                        detail::check_hip(cuddh_hip_stream_sync(stream()), "gmres sync");
                        detail::check_hip(cuddh_hip_copy_d2h_on(h, dcol, sizeof(scalar) * (k1 + 1), stream()), "gmres column copy");
                        h[k1] = std::sqrt(h[k1]); // the reduced sum of squares
                        if (h[k1] != zero)
                            scal(n, one / h[k1], vk1);
                    }
                    else if (ahead)
                    {
                        // one step ahead: step k + 1 is queued (its operator apply needs nothing from the host) before the host waits
                        // for step k's column, so the device never idles while the host rotates; if the iteration stops at column k
                        // the extra step is discarded (it wrote v_{k+2} and the device column, neither is read afterwards)
                        if (k + 1 < m)
                            queue_step(k + 1);
                        detail::check_hip(cuddh_hip_event_sync(ev[k & 1]), "gmres event wait");
                        std::copy(pin[k & 1], pin[k & 1] + k1 + 1, h);
                    }
                    else
                    {
                        queue_step(k);
                        detail::check_hip(cuddh_hip_stream_sync(stream()), "gmres sync");
                        detail::check_hip(cuddh_hip_copy_d2h_on(h, dcol, sizeof(scalar) * (k1 + 1), stream()), "gmres column copy");
                    }
                    if (k < n_krylov)
                        out.num_matvec++;

                    if (h[k1] == zero)
                        break;

                    rotate_column(h, cs.data(), sn.data(), k);
                    eta[k1] = -sn[k] * eta[k];
                    eta[k] = cs[k] * eta[k];

                    if (std::abs(eta[k1]) < tol * bnrm)
                        break;
                }

                back_substitute(k1, H.data(), m1, eta.data());
                scalar dx_nrm = zero;
                if (augment == 0)
                    for (int k = 0; k < k1; ++k)
                        axpby(n, eta[k], V + static_cast<std::size_t>(k) * ldv, one, x);
                else
                {
                    // dx = sum_j y_j u_j (u_j = v_j, then z_p), x <- x + dx and the partial sums of |dx|^2 in one launch
                    const int nv = std::min(k1, n_krylov), nz = k1 - nv;
                    scalar dxx = zero;
                    detail::check_hip(cuddh_hip_copy_h2d_on(d_coef, eta.data(), sizeof(scalar) * k1, stream()), "gmres update coefficients");
                    detail::check_hip(k_update(n, x, dxv, V, static_cast<long long>(ldv), nv, Zs, static_cast<long long>(ldv), nz, d_coef, d_part), "gmres update");
                    detail::check_hip(k_cgs_reduce(n, 0, d_part, d_dxx), "gmres update reduce");
                    if (n == 0) // (a rank without entries: nothing was launched)
                        detail::check_hip(cuddh_hip_copy_h2d_on(d_dxx, &dxx, sizeof(scalar), stream()), "gmres update norm");
                    if (red)
                        red->fn(red->user, d_dxx, 1, is_f64);
                    detail::check_hip(cuddh_hip_stream_sync(stream()), "gmres sync");
                    detail::check_hip(cuddh_hip_copy_d2h_on(&dxx, d_dxx, sizeof(scalar), stream()), "gmres update norm");
                    dx_nrm = std::sqrt(dxx);
                }
                // a new pair: the older ones move back by one place (the oldest of `augment` is dropped), r_old waits in the first
                const bool new_pair = dx_nrm > zero;
                if (new_pair)
                {
                    for (int p = std::min(n_pairs, augment - 1); p >= 1; --p)
                    {
                        copy(n, Zs + static_cast<std::size_t>(p - 1) * ldv, Zs + static_cast<std::size_t>(p) * ldv);
                        copy(n, AZs + static_cast<std::size_t>(p - 1) * ldv, AZs + static_cast<std::size_t>(p) * ldv);
                    }
                    copy(n, r, AZs);
                }

                A->action(x, r);
                out.num_matvec++;
                axpby(n, one, b, -one, r);
                r_nrm = norm_of(r);

                out.res_norm.push_back(static_cast<double>(r_nrm));
                const double elapsed = std::chrono::duration<double>(clock::now() - t0).count();
                out.time.push_back(elapsed);
                bool out_of_time = elapsed > max_seconds;
                if (red)
                {
                    // each rank reads its own clock: the decision to stop must be the same on all of them, or one rank leaves the
                    // sequence of collectives while the others enter the next one -- reduce the flag like every other scalar
                    const scalar flag = out_of_time ? one : zero;
                    scalar total = zero;
                    detail::check_hip(cuddh_hip_copy_h2d_on(dcol, &flag, sizeof(scalar), stream()), "gmres stop flag");
                    red->fn(red->user, dcol, 1, is_f64);
                    detail::check_hip(cuddh_hip_stream_sync(stream()), "gmres sync");
                    detail::check_hip(cuddh_hip_copy_d2h_on(&total, dcol, sizeof(scalar), stream()), "gmres stop flag");
                    out_of_time = total > zero;
                }
                if (out_of_time)
                    break;

                if (verbose == 1)
                {
                    const int width = 30;
                    const int filled = std::min(width, width * it / std::max(1, maxit - 1));
                    std::cout << "[" << std::string(filled, '#') << std::string(width - filled, ' ') << "] || iteration "
                              << std::setw(10) << it + 1 << " / " << maxit << " || rel. res. = " << std::setw(10)
                              << r_nrm / bnrm << "\r" << std::flush;
                }
                else if (verbose >= 2)
                {
                    std::cout << "iteration " << std::setw(10) << it + 1 << " / " << maxit
                              << " || rel. res. = " << std::setw(10) << r_nrm / bnrm << std::endl;
                }

                if (r_nrm < tol * bnrm)
                {
                    out.success = true;
                    break;
                }

                if (new_pair)
                {
                    // another cycle follows: z = dx / |dx|,  A z = (r_old - r_new) / |dx|, no operator application
                    axpby(n, -one / dx_nrm, r, one / dx_nrm, AZs);
                    axpby(n, one / dx_nrm, dxv, zero, Zs);
                    n_pairs = std::min(n_pairs + 1, augment);
                }
            }

            if (verbose == 1)
                std::cout << std::endl;
            if (verbose)
                std::cout << "After " << it << " iterations, GMRES achieved rel. residual of " << out.res_norm.back() / bnrm
                          << (out.success ? "\nGMRES successfully converged within desired tolerance."
                                          : "\nGMRES failed to converge within desired tolerance.")
                          << std::endl;

            out.num_iter = it;
            return out;
        }
        // ---- GMRES(m) over the complex numbers on split [Re; Im] vectors (krylov.hpp: Arithmetic::complex)
        using cplx = std::complex<double>;

        // products and quotients written out (no special-value handling of the library's operators; Smith's division, so that a
        // real divisor divides both parts by it and nothing else)
        inline cplx cmul(cplx a, cplx b) { return {a.real() * b.real() - a.imag() * b.imag(), a.real() * b.imag() + a.imag() * b.real()}; }
        inline cplx cdiv(cplx a, cplx b)
        {
            if (std::abs(b.real()) >= std::abs(b.imag()))
            {
                const double q = b.imag() / b.real(), d = b.real() + b.imag() * q;
                return {(a.real() + a.imag() * q) / d, (a.imag() - a.real() * q) / d};
            }
            const double q = b.real() / b.imag(), d = b.real() * q + b.imag();
            return {(a.real() * q + a.imag()) / d, (a.imag() * q - a.real()) / d};
        }

        // the rotations of rotate_column with complex entries: G_i = [conj(cs_i), conj(sn_i); -sn_i, cs_i], cs_k = h_k / t, sn_k = h_{k+1} / t,
        // t = sqrt(|h_k|^2 + |h_{k+1}|^2) (h_{k+1}, a norm, is real); with real entries these are rotate_column's own operations
        void rotate_column_complex(cplx *h, cplx *cs, cplx *sn, int k)
        {
            for (int i = 0; i < k; ++i)
            {
                const cplx a = h[i], b = h[i + 1];
                h[i] = cmul(std::conj(cs[i]), a) + cmul(std::conj(sn[i]), b);
                h[i + 1] = cmul(cs[i], b) - cmul(sn[i], a);
            }
            const double t = std::hypot(std::hypot(h[k].real(), h[k].imag()), std::hypot(h[k + 1].real(), h[k + 1].imag()));
            cs[k] = {h[k].real() / t, h[k].imag() / t};
            sn[k] = {h[k + 1].real() / t, h[k + 1].imag() / t};
            h[k] = cmul(std::conj(cs[k]), h[k]) + cmul(std::conj(sn[k]), h[k + 1]);
            h[k + 1] = 0;
        }

        template <typename scalar, typename Op>
        solver_out arnoldi_restarted_complex(int n, scalar *x, const Op *A, const scalar *b, int m, int maxit, scalar tol, int verbose,
                                             double max_seconds, const GmresOptions &opt)
        {
            using clock = std::chrono::high_resolution_clock;
            const scalar one = 1, zero = 0;
            const int m1 = m + 1;

            if (opt.orth != Orthogonalization::mgs)
                cuddh_error("gmres error: complex arithmetic needs orthogonalization mgs.");
            if (opt.augment != 0)
                cuddh_error("gmres error: complex arithmetic needs augment = 0.");
            if (n < 0 || n % 2 != 0)
                cuddh_error("gmres error: complex arithmetic needs vectors of an even length (real parts, then imaginary parts).");
            if (m < 1 || m > 512)
                cuddh_error("gmres error: complex arithmetic takes restart lengths from 1 to 512 (one launch of the update covers every column).");
            const int half = n / 2;
            // distance of two basis vectors: n rounded up to 16 bytes (the update reads all of them in one launch)
            constexpr std::size_t per16 = 16 / sizeof(scalar);
            const std::size_t ldv = (static_cast<std::size_t>(n) + per16 - 1) / per16 * per16;

            HostDeviceArray<scalar> r_store(n), V_store(ldv * m1);
            scalar *r = r_store.device_write();
            scalar *V = V_store.device_write();

            // two halves of partial sums (two rows each), the Hessenberg column under construction (re, im interleaved) and the
            // coefficients of the update
            void *ws = nullptr;
            const std::size_t ws_bytes = cuddh_hip_cmgs_ws_bytes();
            detail::check_hip(cuddh_hip_malloc_zeroed(&ws, ws_bytes + (2 * (m1 + 1) + 2 * m) * sizeof(double)), "gmres workspace");
            struct Guard
            {
                void *p;
                ~Guard() { cuddh_hip_free(p); }
            } guard{ws};
            scalar *dcol = reinterpret_cast<scalar *>(static_cast<char *>(ws) + ws_bytes);
            scalar *d_coef = dcol + 2 * (m1 + 1);

            const bool ahead = dynamic_cast<const QueuesDeviceWorkOnly *>(A) != nullptr;
            struct AheadBuffers
            {
                scalar *pin[2] = {nullptr, nullptr};
                void *ev[2] = {nullptr, nullptr};
                ~AheadBuffers()
                {
                    for (int i = 0; i < 2; ++i)
                    {
                        (void)cuddh_hip_host_free(pin[i]);
                        (void)cuddh_hip_event_destroy(ev[i]);
                    }
                }
            } ab;
            if (ahead)
                for (int i = 0; i < 2; ++i)
                {
                    detail::check_hip(cuddh_hip_host_alloc(reinterpret_cast<void **>(&ab.pin[i]), sizeof(scalar) * 2 * (m1 + 1)), "gmres pinned column");
                    detail::check_hip(cuddh_hip_event_create(&ab.ev[i]), "gmres event");
                }
            scalar *const *pin = ab.pin;
            void *const *ev = ab.ev;

            const scalar bnrm = norm(n, b);

            std::vector<cplx> H(static_cast<std::size_t>(m1) * m, cplx(0)), cs(m, cplx(0)), sn(m, cplx(0)), eta(m1, cplx(0));
            std::vector<scalar> col(2 * (m1 + 1), zero), coef(2 * m, zero);

            solver_out out;
            out.success = false;
            out.num_iter = 0;
            out.num_matvec = 0;
            out.res_norm.reserve(maxit + 1);
            out.time.reserve(maxit + 1);

            A->action(x, r);
            out.num_matvec++;
            axpby(n, one, b, -one, r); // r = b - A x
            scalar r_nrm = norm(n, r);

            out.res_norm.push_back(static_cast<double>(r_nrm));
            out.time.push_back(0.0);
            const auto t0 = clock::now();

            if (r_nrm < tol * bnrm)
            {
                out.success = true;
                if (verbose)
                    std::cout << "After 0 iterations, GMRES achieved rel. residual of " << out.res_norm.back() / bnrm
                              << "\nGMRES successfully converged within desired tolerance." << std::endl;
                return out;
            }

            if (verbose)
                std::cout << std::setprecision(5) << std::scientific;

            int it = 1;
            for (; it < maxit; ++it)
            {
                axpby(n, one / r_nrm, r, zero, V); // v0 = r / ||r||
                std::fill(eta.begin(), eta.end(), cplx(0));
                eta[0] = static_cast<double>(r_nrm);

                // One Arnoldi step: the chain of arnoldi_restarted's queue_step with complex coefficients -- stage j applies
                // h_j = <v_{j-1}, w> and leaves the partial sums of <v_j, w>, the last one those of |w|^2 for mgs_finish on the
                // n scalars.  k + 3 launches, as there.  dcol[2 j], dcol[2 j + 1] = h_j; dcol[2 (k + 1)] = |w|.
                auto queue_step = [&](int k)
                {
                    scalar *vk = V + static_cast<std::size_t>(k) * ldv;
                    scalar *vk1 = vk + ldv;
                    A->action(vk, vk1);
                    scalar *pa = static_cast<scalar *>(ws), *pb = pa + ws_bytes / (2 * sizeof(double));
                    detail::check_hip(k_cmgs_stage(half, vk1, static_cast<const scalar *>(nullptr), V, pa, pa, dcol), "gmres complex mgs");
                    for (int j = 0; j <= k; ++j)
                    {
                        const scalar *vj = V + static_cast<std::size_t>(j) * ldv;
                        const scalar *vnext = (j < k) ? vj + ldv : nullptr;
                        detail::check_hip(k_cmgs_stage(half, vk1, vj, vnext, pa, pb, dcol + 2 * j), "gmres complex mgs");
                        std::swap(pa, pb);
                    }
                    detail::check_hip(k_mgs_finish(n, vk1, pa, dcol + 2 * (k + 1)), "gmres normalise");
                    if (ahead)
                    {
                        detail::check_hip(cuddh_hip_copy_d2h_async(pin[k & 1], dcol, sizeof(scalar) * (2 * k + 3), stream()), "gmres column copy");
                        detail::check_hip(cuddh_hip_event_record(ev[k & 1], stream()), "gmres event");
                    }
                };

                int k1 = 0;
                if (ahead)
                    queue_step(0);
                for (int k = 0; k < m; ++k)
                {
                    k1 = k + 1;
                    cplx *h = H.data() + static_cast<std::size_t>(m1) * k;
                    if (ahead)
                    {
                        // one step ahead, as on the real path: the step queued beyond an exit is discarded
                        if (k + 1 < m)
                            queue_step(k + 1);
                        detail::check_hip(cuddh_hip_event_sync(ev[k & 1]), "gmres event wait");
                        std::copy(pin[k & 1], pin[k & 1] + 2 * k + 3, col.data());
                    }
                    else
                    {
                        queue_step(k);
                        detail::check_hip(cuddh_hip_stream_sync(stream()), "gmres sync");
                        detail::check_hip(cuddh_hip_copy_d2h_on(col.data(), dcol, sizeof(scalar) * (2 * k + 3), stream()), "gmres column copy");
                    }
                    out.num_matvec++;
                    for (int j = 0; j < k1; ++j)
                        h[j] = cplx(static_cast<double>(col[2 * j]), static_cast<double>(col[2 * j + 1]));
                    h[k1] = static_cast<double>(col[2 * k1]);

                    if (h[k1] == cplx(0))
                        break;

                    rotate_column_complex(h, cs.data(), sn.data(), k);
                    eta[k1] = -cmul(sn[k], eta[k]);
                    eta[k] = cmul(std::conj(cs[k]), eta[k]);

                    if (std::hypot(eta[k1].real(), eta[k1].imag()) < static_cast<double>(tol * bnrm))
                        break;
                }

                // back substitution R y = g (back_substitute with complex entries), then x <- x + sum_j y_j v_j in one launch
                for (int i = k1 - 1; i >= 0; --i)
                {
                    cplx sacc = eta[i];
                    for (int j = i + 1; j < k1; ++j)
                        sacc -= cmul(H[i + static_cast<std::size_t>(m1) * j], eta[j]);
                    eta[i] = cdiv(sacc, H[i + static_cast<std::size_t>(m1) * i]);
                }
                for (int j = 0; j < k1; ++j)
                {
                    coef[2 * j] = static_cast<scalar>(eta[j].real());
                    coef[2 * j + 1] = static_cast<scalar>(eta[j].imag());
                }
                detail::check_hip(cuddh_hip_copy_h2d_on(d_coef, coef.data(), sizeof(scalar) * 2 * k1, stream()), "gmres update coefficients");
                detail::check_hip(k_cupdate(half, x, V, static_cast<long long>(ldv), k1, d_coef), "gmres complex update");

                A->action(x, r);
                out.num_matvec++;
                axpby(n, one, b, -one, r);
                r_nrm = norm(n, r);

                out.res_norm.push_back(static_cast<double>(r_nrm));
                const double elapsed = std::chrono::duration<double>(clock::now() - t0).count();
                out.time.push_back(elapsed);
                if (elapsed > max_seconds)
                    break;

                if (verbose == 1)
                {
                    const int width = 30;
                    const int filled = std::min(width, width * it / std::max(1, maxit - 1));
                    std::cout << "[" << std::string(filled, '#') << std::string(width - filled, ' ') << "] || iteration "
                              << std::setw(10) << it + 1 << " / " << maxit << " || rel. res. = " << std::setw(10)
                              << r_nrm / bnrm << "\r" << std::flush;
                }
                else if (verbose >= 2)
                {
                    std::cout << "iteration " << std::setw(10) << it + 1 << " / " << maxit
                              << " || rel. res. = " << std::setw(10) << r_nrm / bnrm << std::endl;
                }

                if (r_nrm < tol * bnrm)
                {
                    out.success = true;
                    break;
                }
            }

            if (verbose == 1)
                std::cout << std::endl;
            if (verbose)
                std::cout << "After " << it << " iterations, GMRES achieved rel. residual of " << out.res_norm.back() / bnrm
                          << (out.success ? "\nGMRES successfully converged within desired tolerance."
                                          : "\nGMRES failed to converge within desired tolerance.")
                          << std::endl;

            out.num_iter = it;
            return out;
        }

        [[noreturn]] void refuse_complex(const char *with)
        {
            const std::string msg = std::string("gmres error: complex arithmetic cannot be combined with ") + with + ".";
            cuddh_error(msg.c_str());
            throw std::runtime_error(msg);
        }
    } // namespace

    solver_out gmres(int n, double *x, const Operator *A, const double *b, int m, int maxit, double tol, int verbose,
                     double max_seconds)
    {
        return arnoldi_restarted<double>(n, x, A, b, m, maxit, tol, verbose, max_seconds);
    }

    solver_out gmres(int n, double *x, const Operator *A, const double *b, int m, int maxit, double tol, int verbose,
                     double max_seconds, Orthogonalization orth)
    {
        return arnoldi_restarted<double>(n, x, A, b, m, maxit, tol, verbose, max_seconds, nullptr, orth);
    }

    solver_out gmres(int n, double *x, const Operator *A, const double *b, const Operator *Precond, int m, int maxit,
                     double tol, int verbose, double max_seconds, Orthogonalization orth)
    {
        LeftPreconditioned PA(n, A, Precond);
        host_device_dvec Pb(n);
        double *d_Pb = Pb.device_write();
        Precond->action(b, d_Pb);
        return arnoldi_restarted<double>(n, x, &PA, d_Pb, m, maxit, tol, verbose, max_seconds, nullptr, orth);
    }

    solver_out gmres(int n, float *x, const SinglePrecisionOperator *A, const float *b, int m, int maxit, float tol,
                     int verbose, double max_seconds, Orthogonalization orth)
    {
        return arnoldi_restarted<float>(n, x, A, b, m, maxit, tol, verbose, max_seconds, nullptr, orth);
    }

    solver_out gmres(int n, double *x, const Operator *A, const double *b, int m, int maxit, double tol, int verbose,
                     double max_seconds, const ScalarReduce &reduce, Orthogonalization orth)
    {
        return arnoldi_restarted<double>(n, x, A, b, m, maxit, tol, verbose, max_seconds, reduce.fn ? &reduce : nullptr, orth);
    }

    solver_out gmres(int n, float *x, const SinglePrecisionOperator *A, const float *b, int m, int maxit, float tol, int verbose,
                     double max_seconds, const ScalarReduce &reduce, Orthogonalization orth)
    {
        return arnoldi_restarted<float>(n, x, A, b, m, maxit, tol, verbose, max_seconds, reduce.fn ? &reduce : nullptr, orth);
    }

    solver_out gmres(int n, double *x, const Operator *A, const double *b, int m, int maxit, double tol, int verbose, double max_seconds,
                     const GmresOptions &opt)
    {
        if (opt.arithmetic == Arithmetic::complex)
            return arnoldi_restarted_complex<double>(n, x, A, b, m, maxit, tol, verbose, max_seconds, opt);
        return arnoldi_restarted<double>(n, x, A, b, m, maxit, tol, verbose, max_seconds, nullptr, opt.orth, opt.augment);
    }

    solver_out gmres(int n, double *x, const Operator *A, const double *b, const Operator *Precond, int m, int maxit, double tol, int verbose,
                     double max_seconds, const GmresOptions &opt)
    {
        if (opt.arithmetic == Arithmetic::complex)
            refuse_complex("a preconditioner");
        LeftPreconditioned PA(n, A, Precond);
        host_device_dvec Pb(n);
        double *d_Pb = Pb.device_write();
        Precond->action(b, d_Pb);
        return arnoldi_restarted<double>(n, x, &PA, d_Pb, m, maxit, tol, verbose, max_seconds, nullptr, opt.orth, opt.augment);
    }

    solver_out gmres(int n, float *x, const SinglePrecisionOperator *A, const float *b, int m, int maxit, float tol, int verbose,
                     double max_seconds, const GmresOptions &opt)
    {
        if (opt.arithmetic == Arithmetic::complex)
            return arnoldi_restarted_complex<float>(n, x, A, b, m, maxit, tol, verbose, max_seconds, opt);
        return arnoldi_restarted<float>(n, x, A, b, m, maxit, tol, verbose, max_seconds, nullptr, opt.orth, opt.augment);
    }

    solver_out gmres(int n, double *x, const Operator *A, const double *b, int m, int maxit, double tol, int verbose,
                     double max_seconds, const ScalarReduce &reduce, const GmresOptions &opt)
    {
        if (opt.arithmetic == Arithmetic::complex)
            refuse_complex("partitioned vectors (a ScalarReduce)");
        return arnoldi_restarted<double>(n, x, A, b, m, maxit, tol, verbose, max_seconds, reduce.fn ? &reduce : nullptr, opt.orth, opt.augment);
    }

    solver_out gmres(int n, float *x, const SinglePrecisionOperator *A, const float *b, int m, int maxit, float tol, int verbose,
                     double max_seconds, const ScalarReduce &reduce, const GmresOptions &opt)
    {
        if (opt.arithmetic == Arithmetic::complex)
            refuse_complex("partitioned vectors (a ScalarReduce)");
        return arnoldi_restarted<float>(n, x, A, b, m, maxit, tol, verbose, max_seconds, reduce.fn ? &reduce : nullptr, opt.orth, opt.augment);
    }

    solver_out gmres(int n, double *x, const Operator *A, const double *b, const Operator *Precond, int m, int maxit,
                     double tol, int verbose, double max_seconds)
    {
        LeftPreconditioned PA(n, A, Precond);
        host_device_dvec Pb(n);
        double *d_Pb = Pb.device_write();
        Precond->action(b, d_Pb);
        return arnoldi_restarted<double>(n, x, &PA, d_Pb, m, maxit, tol, verbose, max_seconds);
    }

    solver_out gmres(int n, float *x, const SinglePrecisionOperator *A, const float *b, int m, int maxit, float tol,
                     int verbose, double max_seconds)
    {
        return arnoldi_restarted<float>(n, x, A, b, m, maxit, tol, verbose, max_seconds);
    }

    solver_out gmres(int n, double *x, const Operator *A, const double *b, int m, int maxit, double tol, int verbose,
                     double max_seconds, const ScalarReduce &reduce)
    {
        return arnoldi_restarted<double>(n, x, A, b, m, maxit, tol, verbose, max_seconds, reduce.fn ? &reduce : nullptr);
    }

    solver_out gmres(int n, float *x, const SinglePrecisionOperator *A, const float *b, int m, int maxit, float tol, int verbose,
                     double max_seconds, const ScalarReduce &reduce)
    {
        return arnoldi_restarted<float>(n, x, A, b, m, maxit, tol, verbose, max_seconds, reduce.fn ? &reduce : nullptr);
    }
} // namespace cuddh
