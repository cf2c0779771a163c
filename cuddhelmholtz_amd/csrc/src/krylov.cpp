// Restarted GMRES.  Iteration semantics follow reference source/gmres.cpp:91-235
// (see krylov.hpp); the arithmetic is scheduled differently: the k+1 projection
// coefficients of an Arnoldi step stay on the device (each axpy reads its
// coefficient from device memory) and reach the host in one copy per step.
//
// Shape: one restart loop (restarted), one Arnoldi driver (Arnoldi: the step flavours and the one-step-ahead
// pair), one small problem (gmres_small.hpp).  What real and complex arithmetic do differently is an arithmetic policy
// (RealArithmetic, ComplexArithmetic); every public overload forwards to solve().
#include "cuddh/krylov.hpp"

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <string>
#include <type_traits>

#include "cuddh_hip.h"
#include "gmres_small.hpp"

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

        using small::cplx;

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

        // ---- workspaces
        // one zeroed device allocation, carved up by its owner
        struct DeviceScratch
        {
            void *p = nullptr;
            DeviceScratch() = default;
            DeviceScratch(const DeviceScratch &) = delete;
            DeviceScratch &operator=(const DeviceScratch &) = delete;
            ~DeviceScratch() { cuddh_hip_free(p); }

            void allocate(std::size_t bytes, const char *what) { detail::check_hip(cuddh_hip_malloc_zeroed(&p, bytes), what); }

            template <typename T>
            T *at(std::size_t byte_offset) const
            {
                return reinterpret_cast<T *>(static_cast<char *>(p) + byte_offset);
            }
        };

        // two pinned Hessenberg columns and two events: what driving the device one Arnoldi step ahead of the host needs
        template <typename scalar>
        struct AheadBuffers
        {
            scalar *pin[2] = {nullptr, nullptr};
            void *ev[2] = {nullptr, nullptr};
            AheadBuffers() = default;
            AheadBuffers(const AheadBuffers &) = delete;
            AheadBuffers &operator=(const AheadBuffers &) = delete;
            ~AheadBuffers()
            {
                for (int i = 0; i < 2; ++i)
                {
                    (void)cuddh_hip_host_free(pin[i]);
                    (void)cuddh_hip_event_destroy(ev[i]);
                }
            }

            void allocate(int column_scalars)
            {
                for (int i = 0; i < 2; ++i)
                {
                    detail::check_hip(cuddh_hip_host_alloc(reinterpret_cast<void **>(&pin[i]), sizeof(scalar) * column_scalars), "gmres pinned column");
                    detail::check_hip(cuddh_hip_event_create(&ev[i]), "gmres event");
                }
            }
        };

        // distance of two basis vectors when one launch reads all of them as 16-byte vectors: n rounded up to 16 bytes
        template <typename scalar>
        std::size_t rounded_to_16_bytes(int n)
        {
            constexpr std::size_t per16 = 16 / sizeof(scalar);
            return (static_cast<std::size_t>(n) + per16 - 1) / per16 * per16;
        }

        // ---- arithmetic policies: what GMRES over the reals and over the complex numbers do differently
        // An arithmetic names the host entry type, refuses the arguments it cannot take, owns the device workspaces of a solve
        // (partial sums pa / pb of the MGS chain, the Hessenberg column dcol under construction), says how a fetched column
        // becomes host entries, launches one stage of the MGS chain and ends a cycle (x <- x + sum_j y_j u_j).

        // Real arithmetic, with everything that exists on it only: cgs2, LGMRES augmentation, partitioned vectors.
        template <typename scalar_>
        struct RealArithmetic
        {
            using scalar = scalar_;
            using entry = scalar_;
            static constexpr int is_f64 = sizeof(scalar) == 8;
            static constexpr int entry_scalars = 1; // device scalars per Hessenberg entry
            static constexpr const char *mgs_what = "gmres mgs";

            static void refuse(int n, int m, const GmresOptions &opt)
            {
                if (opt.orth != Orthogonalization::mgs && opt.orth != Orthogonalization::cgs2)
                    cuddh_error("gmres error: orthogonalization must be mgs or cgs2.");
                if (opt.orth == Orthogonalization::cgs2 && m > 512)
                    cuddh_error("gmres error: orthogonalization cgs2 takes restart lengths up to 512 (one launch covers the whole basis).");
                // augment = k > 0 (LGMRES, krylov.hpp): the last k corrections z and their images A z take the place of the last Krylov columns
                if (opt.augment < 0 || (opt.augment > 0 && opt.augment >= m))
                    cuddh_error("gmres error: augment must be in [0, m - 1].");
                if (opt.augment > 0 && m > 512)
                    cuddh_error("gmres error: augment takes restart lengths up to 512 (one launch of the update covers every column).");
            }

            // distance of two basis vectors: n; under cgs2 and with augment > 0 rounded up to 16 bytes
            static std::size_t basis_stride(int n, const GmresOptions &opt)
            {
                return (opt.orth == Orthogonalization::cgs2 || opt.augment > 0) ? rounded_to_16_bytes<scalar>(n) : static_cast<std::size_t>(n);
            }

            static int column_capacity(int m) { return m + 2; }
            static int column_scalars(int k) { return k + 2; }

            RealArithmetic(int n_, int m_, std::size_t ldv_, const ScalarReduce *red_, const GmresOptions &opt)
                : n(n_), m(m_), ldv(ldv_), red(red_), cgs2(opt.orth == Orthogonalization::cgs2), augment(opt.augment), col_store(m_ + 2)
            {
                const int m1 = m + 1;
                dcol = col_store.device_write();
                ws.allocate(cuddh_hip_reduce_ws_bytes(), "gmres workspace");
                pa = static_cast<scalar *>(ws.p);
                pb = pa + cuddh_hip_reduce_ws_bytes() / (2 * sizeof(double));

                // cgs2: two partial-sum buffers (cuddh_hip.h: rows of `row` scalars, <w, w> in row 0), the first pass's coefficients, and for
                // partitioned vectors the second pass's reduced coefficients and a row that holds the reduced <w, w> followed by zeros
                // (a pass and cgs_reduce do nothing on an empty vector, so a rank without entries would send stale coefficients into the sums)
                if (cgs2 && red && n == 0)
                    cuddh_error("gmres error: orthogonalization cgs2 needs at least one entry of the partitioned vectors on every rank.");
                if (cgs2)
                {
                    row = cuddh_hip_cgs_ws_bytes(0) / sizeof(double);
                    const std::size_t pbytes = cuddh_hip_cgs_ws_bytes(m);
                    cgs_ws.allocate(2 * pbytes + (2 * (m1 + 1) + row) * sizeof(double), "gmres cgs2 workspace");
                    pA = cgs_ws.template at<scalar>(0);
                    pB = cgs_ws.template at<scalar>(pbytes);
                    dc1 = cgs_ws.template at<scalar>(2 * pbytes);
                    dc2 = dc1 + (m1 + 1);
                    zrow = dc2 + (m1 + 1);
                    n_part = cuddh_hip_cgs_partials(n);
                }

                // augment: the pairs (z_p, A z_p), most recent first, ldv apart like the basis; the correction of a cycle; on the device the
                // coefficients of the update, a row of partial sums of |dx|^2 (the <w, w> row of a cgs pass) and their sum
                if (augment > 0)
                {
                    Z_store.resize(static_cast<int>(ldv * augment));
                    AZ_store.resize(static_cast<int>(ldv * augment));
                    dx_store.resize(n);
                    Zs = Z_store.device_write();
                    AZs = AZ_store.device_write();
                    dxv = dx_store.device_write();
                    const std::size_t prow = cuddh_hip_cgs_ws_bytes(0);
                    aug_ws.allocate(prow + (m + 1) * sizeof(double), "gmres augmentation workspace");
                    d_part = aug_ws.template at<scalar>(0);
                    d_coef = aug_ws.template at<scalar>(prow);
                    d_dxx = d_coef + m;
                }
            }

            // the fetched column lands in H itself
            scalar *landing(entry *h) { return h; }
            void unpack(entry *, int) {}

            int stage(scalar *w, const scalar *vp, const scalar *vn, const scalar *pi, scalar *po, scalar *h) const { return k_mgs_stage(n, w, vp, vn, pi, po, h); }

            // columns k < n_krylov are Krylov columns (w = A v_k); column n_krylov + p takes w = A z_p from the stored pair: a copy,
            // no operator application (augment = 0: n_krylov = m)
            int n_krylov() const { return m - std::min(augment, n_pairs); }
            const scalar *stored_image(int p) const { return AZs + static_cast<std::size_t>(p) * ldv; }

            // x <- x + sum_j y_j u_j; with augment > 0 the correction and its norm are kept and a new pair begins
            void end_cycle(scalar *x, const scalar *V, const entry *y, int k1, const scalar *r)
            {
                const scalar one = 1, zero = 0;
                dx_nrm = zero;
                if (augment == 0)
                    for (int k = 0; k < k1; ++k)
                        axpby(n, y[k], V + static_cast<std::size_t>(k) * ldv, one, x);
                else
                {
                    // dx = sum_j y_j u_j (u_j = v_j, then z_p), x <- x + dx and the partial sums of |dx|^2 in one launch
                    const int nv = std::min(k1, n_krylov()), nz = k1 - nv;
                    scalar dxx = zero;
                    detail::check_hip(cuddh_hip_copy_h2d_on(d_coef, y, sizeof(scalar) * k1, stream()), "gmres update coefficients");
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
                new_pair = dx_nrm > zero;
                if (new_pair)
                {
                    for (int p = std::min(n_pairs, augment - 1); p >= 1; --p)
                    {
                        copy(n, Zs + static_cast<std::size_t>(p - 1) * ldv, Zs + static_cast<std::size_t>(p) * ldv);
                        copy(n, AZs + static_cast<std::size_t>(p - 1) * ldv, AZs + static_cast<std::size_t>(p) * ldv);
                    }
                    copy(n, r, AZs);
                }
            }

            // another cycle follows: z = dx / |dx|,  A z = (r_old - r_new) / |dx|, no operator application
            void before_next_cycle(const scalar *r)
            {
                const scalar one = 1, zero = 0;
                if (new_pair)
                {
                    axpby(n, -one / dx_nrm, r, one / dx_nrm, AZs);
                    axpby(n, one / dx_nrm, dxv, zero, Zs);
                    n_pairs = std::min(n_pairs + 1, augment);
                }
            }

            const int n, m;
            const std::size_t ldv;
            const ScalarReduce *const red;
            const bool cgs2;
            const int augment;
            HostDeviceArray<scalar> col_store, Z_store, AZ_store, dx_store;
            DeviceScratch ws, cgs_ws, aug_ws;
            scalar *dcol = nullptr, *pa = nullptr, *pb = nullptr;
            // cgs2
            std::size_t row = 0;
            scalar *pA = nullptr, *pB = nullptr, *dc1 = nullptr, *dc2 = nullptr, *zrow = nullptr;
            int n_part = 0;
            // augment
            scalar *Zs = nullptr, *AZs = nullptr, *dxv = nullptr, *d_part = nullptr, *d_coef = nullptr, *d_dxx = nullptr;
            int n_pairs = 0;
            scalar dx_nrm = 0;
            bool new_pair = false;
        };

        // GMRES(m) over the complex numbers on split [Re; Im] vectors (krylov.hpp: Arithmetic::complex): std::complex<double> on the
        // host whatever the vectors' type; dcol[2 j], dcol[2 j + 1] = h_j; dcol[2 (k + 1)] = |w|
        template <typename scalar_>
        struct ComplexArithmetic
        {
            using scalar = scalar_;
            using entry = cplx;
            static constexpr int is_f64 = sizeof(scalar) == 8;
            static constexpr int entry_scalars = 2;
            static constexpr const char *mgs_what = "gmres complex mgs";

            static void refuse(int n, int m, const GmresOptions &opt)
            {
                if (opt.orth != Orthogonalization::mgs)
                    cuddh_error("gmres error: complex arithmetic needs orthogonalization mgs.");
                if (opt.augment != 0)
                    cuddh_error("gmres error: complex arithmetic needs augment = 0.");
                if (n < 0 || n % 2 != 0)
                    cuddh_error("gmres error: complex arithmetic needs vectors of an even length (real parts, then imaginary parts).");
                if (m < 1 || m > 512)
                    cuddh_error("gmres error: complex arithmetic takes restart lengths from 1 to 512 (one launch of the update covers every column).");
            }

            // distance of two basis vectors: n rounded up to 16 bytes (the update reads all of them in one launch)
            static std::size_t basis_stride(int n, const GmresOptions &) { return rounded_to_16_bytes<scalar>(n); }

            static int column_capacity(int m) { return 2 * (m + 2); }
            static int column_scalars(int k) { return 2 * k + 3; }

            ComplexArithmetic(int n_, int m_, std::size_t ldv_, const ScalarReduce *, const GmresOptions &)
                : n(n_), m(m_), half(n_ / 2), ldv(ldv_), col(2 * (m_ + 2), scalar(0)), coef(2 * m_, scalar(0))
            {
                // two halves of partial sums (two rows each), the Hessenberg column under construction (re, im interleaved) and the
                // coefficients of the update
                const int m1 = m + 1;
                const std::size_t ws_bytes = cuddh_hip_cmgs_ws_bytes();
                ws.allocate(ws_bytes + (2 * (m1 + 1) + 2 * m) * sizeof(double), "gmres workspace");
                pa = static_cast<scalar *>(ws.p);
                pb = pa + ws_bytes / (2 * sizeof(double));
                dcol = ws.template at<scalar>(ws_bytes);
                d_coef = dcol + 2 * (m1 + 1);
            }

            // the fetched column lands in `col` as re / im pairs followed by the real norm
            scalar *landing(entry *) { return col.data(); }
            void unpack(entry *h, int k1)
            {
                for (int j = 0; j < k1; ++j)
                    h[j] = cplx(static_cast<double>(col[2 * j]), static_cast<double>(col[2 * j + 1]));
                h[k1] = static_cast<double>(col[2 * k1]);
            }

            int stage(scalar *w, const scalar *vp, const scalar *vn, const scalar *pi, scalar *po, scalar *c) const { return k_cmgs_stage(half, w, vp, vn, pi, po, c); }

            int n_krylov() const { return m; }
            const scalar *stored_image(int) const { return nullptr; } // (no augmentation: never asked for)

            // x <- x + sum_j y_j v_j in one launch
            void end_cycle(scalar *x, const scalar *V, const entry *y, int k1, const scalar *)
            {
                for (int j = 0; j < k1; ++j)
                {
                    coef[2 * j] = static_cast<scalar>(y[j].real());
                    coef[2 * j + 1] = static_cast<scalar>(y[j].imag());
                }
                detail::check_hip(cuddh_hip_copy_h2d_on(d_coef, coef.data(), sizeof(scalar) * 2 * k1, stream()), "gmres update coefficients");
                detail::check_hip(k_cupdate(half, x, V, static_cast<long long>(ldv), k1, d_coef), "gmres complex update");
            }

            void before_next_cycle(const scalar *) {}

            const int n, m, half;
            const std::size_t ldv;
            DeviceScratch ws;
            scalar *dcol = nullptr, *pa = nullptr, *pb = nullptr, *d_coef = nullptr;
            std::vector<scalar> col, coef;
        };

        // ---- the Arnoldi driver: one column of the Hessenberg matrix per call, by the flavour picked before the cycles start
        template <typename Arith, typename Op>
        struct Arnoldi
        {
            using scalar = typename Arith::scalar;
            using entry = typename Arith::entry;
            static constexpr int is_f64 = Arith::is_f64;
            static constexpr int es = Arith::entry_scalars;

            Arnoldi(Arith &ar_, const Op *A_, scalar *V_, const ScalarReduce *red_)
                : ar(ar_), A(A_), V(V_), n(ar_.n), m(ar_.m), ldv(ar_.ldv), dcol(ar_.dcol), red(red_),
                  // Operators that only queue device work (operator.hpp: QueuesDeviceWorkOnly) are driven one Arnoldi step ahead of the host
                  ahead(!red_ && dynamic_cast<const QueuesDeviceWorkOnly *>(A_) != nullptr)
            {
                if (ahead)
                    ab.allocate(Arith::column_capacity(m));
                if constexpr (std::is_same<Arith, RealArithmetic<scalar>>::value)
                {
                    orthogonalise = ar.cgs2 ? &Arnoldi::cgs2_passes : &Arnoldi::mgs_chain;
                    column = red ? (ar.cgs2 ? &Arnoldi::reduced_cgs2_column : &Arnoldi::reduced_mgs_column) : ahead ? &Arnoldi::ahead_column : &Arnoldi::strict_column;
                }
                else
                {
                    orthogonalise = &Arnoldi::mgs_chain;
                    column = ahead ? &Arnoldi::ahead_column : &Arnoldi::strict_column;
                }
            }

            /// a cycle begins (v_0 is in place): n_krylov is fixed for it, and one step ahead means step 0 is queued now
            void begin_cycle()
            {
                n_krylov = ar.n_krylov();
                if (ahead)
                    queue_step(0);
            }

            /// column k of the Hessenberg matrix into h (k + 2 entries), v_{k+1} into the basis
            void next_column(int k, entry *h) { (this->*column)(k, h); }

            bool is_krylov(int k) const { return k < n_krylov; }

        private:
            scalar *v(int k) const { return V + static_cast<std::size_t>(k) * ldv; }

            // ---- step flavours
            // w = A v_k, or a copy of the stored A z_p
            void next_w(int k, const scalar *vk, scalar *vk1)
            {
                if (k < n_krylov)
                    A->action(vk, vk1);
                else
                    copy(n, ar.stored_image(k - n_krylov), vk1);
            }

            // modified Gram-Schmidt against v_0..v_k as a chain of fused stages (stage j applies the projection on v_{j-1} and leaves
            // the partial sums of <w, v_j> -- the last one <w, w> -- for the next stage, so one launch per basis vector does what
            // dot + reduce + axpy did; coefficients stay on the device), normalisation: k + 3 launches.  On breakdown (norm == 0)
            // v_{k+1} becomes non-finite but is never used.  Complex arithmetic: stage j applies h_j = <v_{j-1}, w> and leaves the
            // partial sums of <v_j, w>, the last one those of |w|^2 for mgs_finish on the n scalars.
            void mgs_chain(int k, scalar *vk1)
            {
                scalar *pa = ar.pa, *pb = ar.pb;
                detail::check_hip(ar.stage(vk1, static_cast<const scalar *>(nullptr), V, pa, pa, dcol), Arith::mgs_what);
                for (int j = 0; j <= k; ++j)
                {
                    const scalar *vj = v(j);
                    const scalar *vnext = (j < k) ? vj + ldv : nullptr;
                    detail::check_hip(ar.stage(vk1, vj, vnext, pa, pb, dcol + es * j), Arith::mgs_what);
                    std::swap(pa, pb);
                }
                detail::check_hip(k_mgs_finish(n, vk1, pa, dcol + es * (k + 1)), "gmres normalise");
            }

            // one pass of classical Gram-Schmidt against all of v_0..v_k at once
            void cgs_pass(int k1, scalar *vk1, int update, int dots, const scalar *cin, int ncin, long long cstride, const scalar *hacc, scalar *hout, scalar *pout)
            {
                detail::check_hip(k_cgs_pass(n, vk1, V, ldv, k1, update, dots, cin, ncin, cstride, hacc, hout, pout), "gmres cgs2 pass");
            }

            // cgs2: classical Gram-Schmidt twice -- pass A the k + 1 inner products, pass B the projection with their sums and the
            // inner products of the result, pass C the projection with those (h_j = c1_j + c2_j) and <w, w>, then the same
            // normalisation: four launches at every k
            void cgs2_passes(int k, scalar *vk1)
            {
                const int k1 = k + 1;
                const scalar *none = nullptr;
                cgs_pass(k1, vk1, 0, 1, none, 0, 0, none, nullptr, ar.pA);
                cgs_pass(k1, vk1, 1, 1, ar.pA + ar.row, ar.n_part, ar.row, none, ar.dc1, ar.pB);
                cgs_pass(k1, vk1, 1, 2, ar.pB + ar.row, ar.n_part, ar.row, ar.dc1, dcol, ar.pA);
                detail::check_hip(k_mgs_finish(n, vk1, ar.pA, dcol + k1), "gmres normalise");
            }

            // One Arnoldi step queued on the stream.  One step ahead: the Hessenberg column leaves for pinned host memory behind the
            // step; the next step may be queued behind it
            void queue_step(int k)
            {
                next_w(k, v(k), v(k + 1));
                (this->*orthogonalise)(k, v(k + 1));
                if (ahead)
                {
                    detail::check_hip(cuddh_hip_copy_d2h_async(ab.pin[k & 1], dcol, sizeof(scalar) * Arith::column_scalars(k), stream()), "gmres column copy");
                    detail::check_hip(cuddh_hip_event_record(ab.ev[k & 1], stream()), "gmres event");
                }
            }

            // the device column of step k, complete on the stream, becomes host entries
            void fetch(int k, entry *h)
            {
                detail::check_hip(cuddh_hip_stream_sync(stream()), "gmres sync");
                detail::check_hip(cuddh_hip_copy_d2h_on(ar.landing(h), dcol, sizeof(scalar) * Arith::column_scalars(k), stream()), "gmres column copy");
                ar.unpack(h, k + 1);
            }

            // ---- column flavours
            void strict_column(int k, entry *h)
            {
                queue_step(k);
                fetch(k, h);
            }

            // one step ahead: step k + 1 is queued (its operator apply needs nothing from the host) before the host waits for step
            // k's column, so the device never idles while the host rotates; if the iteration stops at column k the extra step is
            // discarded (it wrote v_{k+2} and the device column, neither is read afterwards)
            void ahead_column(int k, entry *h)
            {
                if (k + 1 < m)
                    queue_step(k + 1);
                detail::check_hip(cuddh_hip_event_sync(ab.ev[k & 1]), "gmres event wait");
                std::copy(ab.pin[k & 1], ab.pin[k & 1] + Arith::column_scalars(k), ar.landing(h));
                ar.unpack(h, k + 1);
            }

            // partitioned vectors: every coefficient is summed over the ranks before it is applied
            void reduced_mgs_column(int k, entry *h)
            {
                const scalar one = 1, zero = 0;
                const int k1 = k + 1;
                scalar *vk1 = v(k1);
                next_w(k, v(k), vk1);
                for (int j = 0; j < k1; ++j)
                {
                    const scalar *vj = v(j);
                    detail::check_hip(k_dot(n, vk1, vj, dcol + j, ar.ws.p), "gmres dot");
                    red->fn(red->user, dcol + j, 1, is_f64);
                    detail::check_hip(k_axpby_dev(n, -one, dcol + j, vj, one, vk1), "gmres projection");
                }
                detail::check_hip(k_dot(n, vk1, vk1, dcol + k1, ar.ws.p), "gmres dot");
                red->fn(red->user, dcol + k1, 1, is_f64);
                fetch(k, h);
                h[k1] = std::sqrt(h[k1]); // the reduced sum of squares
                if (h[k1] != zero)
                    scal(n, one / h[k1], vk1);
            }

            // partitioned vectors: the k + 1 sums of a pass are reduced over the ranks in one call, and the next pass reads the reduced
            // coefficients (ncin = 1); three reductions per step
            void reduced_cgs2_column(int k, entry *h)
            {
                const int k1 = k + 1;
                scalar *vk1 = v(k1);
                next_w(k, v(k), vk1);
                const scalar *none = nullptr;
                cgs_pass(k1, vk1, 0, 1, none, 0, 0, none, nullptr, ar.pA);
                detail::check_hip(k_cgs_reduce(n, k1, ar.pA, dcol), "gmres cgs2 reduce");
                red->fn(red->user, dcol, k1, is_f64);
                cgs_pass(k1, vk1, 1, 1, dcol, 1, 1, none, ar.dc1, ar.pB);
                detail::check_hip(k_cgs_reduce(n, k1, ar.pB, ar.dc2), "gmres cgs2 reduce");
                red->fn(red->user, ar.dc2, k1, is_f64);
                cgs_pass(k1, vk1, 1, 2, ar.dc2, 1, 1, ar.dc1, dcol, ar.pA);
                detail::check_hip(k_cgs_reduce(n, 0, ar.pA, ar.zrow), "gmres cgs2 reduce"); // zrow[0] = <w, w> of this rank; zeros behind it
                red->fn(red->user, ar.zrow, 1, is_f64);
                detail::check_hip(k_mgs_finish(n, vk1, ar.zrow, dcol + k1), "gmres normalise");
                fetch(k, h);
            }

            Arith &ar;
            const Op *const A;
            scalar *const V;
            const int n, m;
            const std::size_t ldv;
            scalar *const dcol;
            const ScalarReduce *const red;
            const bool ahead;
            AheadBuffers<scalar> ab;
            int n_krylov = 0;
            void (Arnoldi::*orthogonalise)(int, scalar *) = nullptr;
            void (Arnoldi::*column)(int, entry *) = nullptr;
        };

        // ---- the restart loop
        template <typename Arith, typename Op>
        solver_out restarted(int n, typename Arith::scalar *x, const Op *A, const typename Arith::scalar *b, int m, int maxit, typename Arith::scalar tol,
                             int verbose, double max_seconds, const ScalarReduce *red, const GmresOptions &opt)
        {
            using scalar = typename Arith::scalar;
            using entry = typename Arith::entry;
            using clock = std::chrono::high_resolution_clock;
            const scalar one = 1, zero = 0;
            const int m1 = m + 1;
            constexpr int is_f64 = Arith::is_f64;

            Arith::refuse(n, m, opt);
            const std::size_t ldv = Arith::basis_stride(n, opt);

            HostDeviceArray<scalar> r_store(n), V_store(ldv * m1);
            scalar *r = r_store.device_write();
            scalar *V = V_store.device_write();
            Arith ar(n, m, ldv, red, opt);
            scalar *dcol = ar.dcol;
            Arnoldi<Arith, Op> arnoldi(ar, A, V, red);

            // 2-norm; with partitioned vectors the sum of squares is reduced over the ranks first
            auto norm_of = [&](const scalar *v) -> scalar
            {
                if (!red)
                    return norm(n, v);
                scalar ss = 0;
                detail::check_hip(k_dot(n, v, v, dcol, ar.ws.p), "gmres norm");
                red->fn(red->user, dcol, 1, is_f64);
                detail::check_hip(cuddh_hip_stream_sync(stream()), "gmres sync");
                detail::check_hip(cuddh_hip_copy_d2h_on(&ss, dcol, sizeof(scalar), stream()), "gmres norm copy");
                return std::sqrt(ss);
            };

            const scalar bnrm = norm_of(b);

            GmresSmall<entry> lsq(m);
            using real = typename GmresSmall<entry>::real;

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
                lsq.start(static_cast<real>(r_nrm));
                arnoldi.begin_cycle();

                int k1 = 0;
                for (int k = 0; k < m; ++k)
                {
                    k1 = k + 1;
                    entry *h = lsq.column(k);
                    arnoldi.next_column(k, h);
                    if (arnoldi.is_krylov(k))
                        out.num_matvec++;

                    if (h[k1] == entry(0))
                        break;

                    if (lsq.push(k) < static_cast<real>(tol * bnrm))
                        break;
                }

                ar.end_cycle(x, V, lsq.solve(k1), k1, r);

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

                ar.before_next_cycle(r);
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

        // ---- what every public overload forwards to.  Precond: null, or the left preconditioner (P A x = P b).  reduce: null, or the
        // caller's ScalarReduce (one without a function means vectors that are not partitioned).
        template <typename scalar, typename Op>
        solver_out solve(int n, scalar *x, const Op *A, const scalar *b, const Operator *Precond, int m, int maxit, scalar tol, int verbose,
                         double max_seconds, const ScalarReduce *reduce, const GmresOptions &opt)
        {
            const bool complex = opt.arithmetic == Arithmetic::complex;
            if (complex && Precond)
                refuse_complex("a preconditioner");
            if (complex && reduce)
                refuse_complex("partitioned vectors (a ScalarReduce)");
            const ScalarReduce *red = (reduce && reduce->fn) ? reduce : nullptr;
            if constexpr (std::is_same<Op, Operator>::value)
                if (Precond)
                {
                    LeftPreconditioned PA(n, A, Precond);
                    host_device_dvec Pb(n);
                    double *d_Pb = Pb.device_write();
                    Precond->action(b, d_Pb);
                    return restarted<RealArithmetic<double>, Operator>(n, x, &PA, d_Pb, m, maxit, tol, verbose, max_seconds, red, opt);
                }
            if (complex)
                return restarted<ComplexArithmetic<scalar>>(n, x, A, b, m, maxit, tol, verbose, max_seconds, red, opt);
            return restarted<RealArithmetic<scalar>>(n, x, A, b, m, maxit, tol, verbose, max_seconds, red, opt);
        }

        // GmresSmall on host arrays: columns in, coefficients and estimates out (complex entries are re, im pairs of doubles)
        template <typename entry, typename stored>
        void run_small(int m, int ncols, const stored *cols, double beta, stored *y_out, double *est_out)
        {
            GmresSmall<entry> lsq(m);
            lsq.start(static_cast<typename GmresSmall<entry>::real>(beta));
            for (int k = 0; k < ncols; cols += (k + 2) * (sizeof(entry) / sizeof(stored)), ++k)
            {
                std::memcpy(lsq.column(k), cols, sizeof(entry) * (k + 2));
                est_out[k] = static_cast<double>(lsq.push(k));
            }
            std::memcpy(y_out, lsq.solve(ncols), sizeof(entry) * ncols);
        }
    } // namespace

    bool gmres_small_problem(int is_complex, int is_f64, int m, int ncols, const void *h_cols, double beta, void *y_out, double *est_out)
    {
        if (m < 1 || ncols < 1 || ncols > m || !h_cols || !y_out || !est_out)
            return false;
        if (is_complex)
            run_small<cplx>(m, ncols, static_cast<const double *>(h_cols), beta, static_cast<double *>(y_out), est_out);
        else if (is_f64)
            run_small<double>(m, ncols, static_cast<const double *>(h_cols), beta, static_cast<double *>(y_out), est_out);
        else
            run_small<float>(m, ncols, static_cast<const float *>(h_cols), beta, static_cast<float *>(y_out), est_out);
        return true;
    }

    // ---- the reference's three
    solver_out gmres(int n, double *x, const Operator *A, const double *b, const Operator *Precond, int m, int maxit, double tol, int verbose, double max_seconds)
    {
        return solve(n, x, A, b, Precond, m, maxit, tol, verbose, max_seconds, nullptr, GmresOptions());
    }

    solver_out gmres(int n, double *x, const Operator *A, const double *b, int m, int maxit, double tol, int verbose, double max_seconds)
    {
        return solve(n, x, A, b, nullptr, m, maxit, tol, verbose, max_seconds, nullptr, GmresOptions());
    }

    solver_out gmres(int n, float *x, const SinglePrecisionOperator *A, const float *b, int m, int maxit, float tol, int verbose, double max_seconds)
    {
        return solve(n, x, A, b, nullptr, m, maxit, tol, verbose, max_seconds, nullptr, GmresOptions());
    }

    // ---- partitioned vectors
    solver_out gmres(int n, double *x, const Operator *A, const double *b, int m, int maxit, double tol, int verbose, double max_seconds, const ScalarReduce &reduce)
    {
        return solve(n, x, A, b, nullptr, m, maxit, tol, verbose, max_seconds, &reduce, GmresOptions());
    }

    solver_out gmres(int n, float *x, const SinglePrecisionOperator *A, const float *b, int m, int maxit, float tol, int verbose, double max_seconds, const ScalarReduce &reduce)
    {
        return solve(n, x, A, b, nullptr, m, maxit, tol, verbose, max_seconds, &reduce, GmresOptions());
    }

    // ---- a chosen orthogonalisation
    solver_out gmres(int n, double *x, const Operator *A, const double *b, const Operator *Precond, int m, int maxit, double tol, int verbose, double max_seconds, Orthogonalization orth)
    {
        return solve(n, x, A, b, Precond, m, maxit, tol, verbose, max_seconds, nullptr, GmresOptions{orth});
    }

    solver_out gmres(int n, double *x, const Operator *A, const double *b, int m, int maxit, double tol, int verbose, double max_seconds, Orthogonalization orth)
    {
        return solve(n, x, A, b, nullptr, m, maxit, tol, verbose, max_seconds, nullptr, GmresOptions{orth});
    }

    solver_out gmres(int n, float *x, const SinglePrecisionOperator *A, const float *b, int m, int maxit, float tol, int verbose, double max_seconds, Orthogonalization orth)
    {
        return solve(n, x, A, b, nullptr, m, maxit, tol, verbose, max_seconds, nullptr, GmresOptions{orth});
    }

    solver_out gmres(int n, double *x, const Operator *A, const double *b, int m, int maxit, double tol, int verbose, double max_seconds, const ScalarReduce &reduce, Orthogonalization orth)
    {
        return solve(n, x, A, b, nullptr, m, maxit, tol, verbose, max_seconds, &reduce, GmresOptions{orth});
    }

    solver_out gmres(int n, float *x, const SinglePrecisionOperator *A, const float *b, int m, int maxit, float tol, int verbose, double max_seconds, const ScalarReduce &reduce, Orthogonalization orth)
    {
        return solve(n, x, A, b, nullptr, m, maxit, tol, verbose, max_seconds, &reduce, GmresOptions{orth});
    }

    // ---- GmresOptions
    solver_out gmres(int n, double *x, const Operator *A, const double *b, const Operator *Precond, int m, int maxit, double tol, int verbose, double max_seconds, const GmresOptions &opt)
    {
        return solve(n, x, A, b, Precond, m, maxit, tol, verbose, max_seconds, nullptr, opt);
    }

    solver_out gmres(int n, double *x, const Operator *A, const double *b, int m, int maxit, double tol, int verbose, double max_seconds, const GmresOptions &opt)
    {
        return solve(n, x, A, b, nullptr, m, maxit, tol, verbose, max_seconds, nullptr, opt);
    }

    solver_out gmres(int n, float *x, const SinglePrecisionOperator *A, const float *b, int m, int maxit, float tol, int verbose, double max_seconds, const GmresOptions &opt)
    {
        return solve(n, x, A, b, nullptr, m, maxit, tol, verbose, max_seconds, nullptr, opt);
    }

    solver_out gmres(int n, double *x, const Operator *A, const double *b, int m, int maxit, double tol, int verbose, double max_seconds, const ScalarReduce &reduce, const GmresOptions &opt)
    {
        return solve(n, x, A, b, nullptr, m, maxit, tol, verbose, max_seconds, &reduce, opt);
    }

    solver_out gmres(int n, float *x, const SinglePrecisionOperator *A, const float *b, int m, int maxit, float tol, int verbose, double max_seconds, const ScalarReduce &reduce, const GmresOptions &opt)
    {
        return solve(n, x, A, b, nullptr, m, maxit, tol, verbose, max_seconds, &reduce, opt);
    }
} // namespace cuddh
