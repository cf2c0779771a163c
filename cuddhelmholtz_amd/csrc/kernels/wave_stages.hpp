// The pointwise arithmetic of the whole-domain WaveHoltz march, shared by its two kernel files: waveholtz.hip (the stages behind a
// stiffness apply, w = K p' read from memory) and wave_lattice.hip (the same stages with w computed in the launch).  The stage
// formulas are stated at the head of waveholtz.hip.  Every product-sum is an explicit fused multiply-add in a fixed order.
// The stages are templates on the scalar R: double for those two files (Begin, Rk2A, ... name the double forms), float for
// wave_lattice_f32.hip, which then rounds like them operation by operation.
// The kernels' stage arguments (StageArgsT<R>, MAX_IN inputs, MAX_OUT outputs, MAX_COEF scalars) and the host code that fills them
// are in wave_sweep_launch.hpp.
#ifndef CUDDH_AMD_WAVE_STAGES_HPP
#define CUDDH_AMD_WAVE_STAGES_HPP

#include "common.hpp"

namespace cuddh_k
{
    namespace wave
    {
        constexpr long long NT_BYTES = 64LL << 20; // vectors from this size on are streamed non-temporally
        constexpr int MAX_IN = 12, MAX_OUT = 4, MAX_COEF = 4;

        using V2 = double __attribute__((ext_vector_type(2)));

        __device__ inline double fmadd(double a, double b, double c) { return __builtin_fma(a, b, c); }
        __device__ inline float fmadd(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

        // invm * (w - Hi q + c F + s G); fg points at (F, G) of this element
        template <bool FORCED, typename R>
        __device__ inline R fq(R w, R q, R invm, R Hi, const R *fg, R c, R s)
        {
            R r = fmadd(-Hi, q, w);
            if constexpr (FORCED)
            {
                r = fmadd(c, fg[0], r);
                r = fmadd(s, fg[1], r);
            }
            return invm * r;
        }

        // A stage: NIN inputs besides (F, G), which follow them when FORCED; NOUT outputs; apply() on one element.
        template <typename R>
        struct BeginT
        {
            static constexpr int NIN = 2, NOUT = 4; // in: zu zv; out: p q u v; coef: filt0
            template <bool FORCED>
            __device__ static void apply(const R *x, R *y, const R *k)
            {
                y[0] = x[0];
                y[1] = x[1];
                y[2] = k[0] * x[0];
                y[3] = k[0] * x[1];
            }
        };
        template <typename R>
        struct Rk2AT
        {
            static constexpr int NIN = 5, NOUT = 2; // in: w p q invm Hi; out: qh ph; coef: dt/2 c s
            template <bool FORCED>
            __device__ static void apply(const R *x, R *y, const R *k)
            {
                y[0] = fmadd(k[0], fq<FORCED>(x[0], x[2], x[3], x[4], x + NIN, k[1], k[2]), x[2]);
                y[1] = fmadd(-k[0], x[2], x[1]);
            }
        };
        template <typename R>
        struct Rk2BT
        {
            static constexpr int NIN = 8, NOUT = 4; // in: w qh p q u v invm Hi; out: p q u v; coef: dt c s filt
            template <bool FORCED>
            __device__ static void apply(const R *x, R *y, const R *k)
            {
                const R p = fmadd(-k[0], x[1], x[2]);
                const R q = fmadd(k[0], fq<FORCED>(x[0], x[1], x[6], x[7], x + NIN, k[1], k[2]), x[3]);
                y[0] = p;
                y[1] = q;
                y[2] = fmadd(k[3], p, x[4]);
                y[3] = fmadd(k[3], q, x[5]);
            }
        };
        template <typename R>
        struct Rk4FirstT
        {
            static constexpr int NIN = 5, NOUT = 4; // in: w p q invm Hi; out: ps qs aq ap; coef: dt/2 c s
            template <bool FORCED>
            __device__ static void apply(const R *x, R *y, const R *k)
            {
                const R kq = fq<FORCED>(x[0], x[2], x[3], x[4], x + NIN, k[1], k[2]);
                y[0] = fmadd(-k[0], x[2], x[1]);
                y[1] = fmadd(k[0], kq, x[2]);
                y[2] = kq;
                y[3] = -x[2];
            }
        };
        template <typename R>
        struct Rk4MidT
        {
            static constexpr int NIN = 8, NOUT = 4; // in: w p q qs aq ap invm Hi; out: ps qs aq ap; coef: h c s  (h = dt/2, then dt)
            template <bool FORCED>
            __device__ static void apply(const R *x, R *y, const R *k)
            {
                const R kq = fq<FORCED>(x[0], x[3], x[6], x[7], x + NIN, k[1], k[2]);
                y[0] = fmadd(-k[0], x[3], x[1]);
                y[1] = fmadd(k[0], kq, x[2]);
                y[2] = fmadd(R(2), kq, x[4]);
                y[3] = fmadd(R(-2), x[3], x[5]);
            }
        };
        template <typename R>
        struct Rk4LastT
        {
            static constexpr int NIN = 10, NOUT = 4; // in: w p q qs aq ap u v invm Hi; out: p q u v; coef: dt/6 c s filt
            template <bool FORCED>
            __device__ static void apply(const R *x, R *y, const R *k)
            {
                const R kq = fq<FORCED>(x[0], x[3], x[8], x[9], x + NIN, k[1], k[2]);
                const R p = fmadd(k[0], x[5] - x[3], x[1]);
                const R q = fmadd(k[0], x[4] + kq, x[2]);
                y[0] = p;
                y[1] = q;
                y[2] = fmadd(k[3], p, x[6]);
                y[3] = fmadd(k[3], q, x[7]);
            }
        };

        using Begin = BeginT<double>;
        using Rk2A = Rk2AT<double>;
        using Rk2B = Rk2BT<double>;
        using Rk4First = Rk4FirstT<double>;
        using Rk4Mid = Rk4MidT<double>;
        using Rk4Last = Rk4LastT<double>;

        template <bool NT, typename V>
        __device__ inline V stream_load(const V *p)
        {
            if constexpr (NT)
                return __builtin_nontemporal_load(p);
            else
                return *p;
        }
        template <bool NT, typename V>
        __device__ inline void stream_store(V *p, const V &v)
        {
            if constexpr (NT)
                __builtin_nontemporal_store(v, p);
            else
                *p = v;
        }

        inline bool aligned16(const void *p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }
    } // namespace wave
} // namespace cuddh_k

#endif
