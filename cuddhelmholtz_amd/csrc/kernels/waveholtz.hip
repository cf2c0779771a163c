// Stage kernels of the whole-domain WaveHoltz march (csrc/src/waveholtz.cpp): everything a Runge-Kutta sweep does
// besides its stiffness apply, in ONE launch per sweep, every vector read once and written once.
//
// State: p, q (the wave and its time derivative's negative, tests/ddh_rk.py), u, v (the filtered period average).  With
//   fq(k; w, q) = invm * (w - Hi q + cs[k] F + sn[k] G),   w = K p' the sweep just applied,
// the stages are
//   begin:  p = zu, q = zv, u = filt[0] zu, v = filt[0] zv
//   rk2_a:  qh = q + dt/2 fq(w, q),  ph = p - dt/2 q                                            (w = K p)
//   rk2_b:  p -= dt qh,  q += dt fq(w, qh),  u += filt p,  v += filt q                          (w = K ph)
//   rk4_1:  k = fq(w, q);   ps = p - dt/2 q,   qs = q + dt/2 k,  aq = k,        ap = -q         (w = K p)
//   rk4_2:  k = fq(w, qs);  ps = p - dt/2 qs,  qs = q + dt/2 k,  aq += 2 k,     ap -= 2 qs      (w = K ps)
//   rk4_3:  k = fq(w, qs);  ps = p - dt qs,    qs = q + dt k,    aq += 2 k,     ap -= 2 qs      (w = K ps; rk4_2 with dt for dt/2)
//   rk4_4:  k = fq(w, qs);  p += dt/6 (ap - qs),  q += dt/6 (aq + k),  u += filt p,  v += filt q
// cs[k], sn[k], filt[it] and dt are kernel arguments: the march reads no device table.  FORCED = false is the homogeneous form (the
// GMRES action): F and G are not arguments of that instantiation.  Every product-sum is an explicit fused multiply-add in a fixed
// order, so that the forced form with F = G = 0 gives the homogeneous form's numbers.
//
// Access pattern: blas1.hip's (contiguous tiles of 16-byte vectors taken in order by the workgroups, clamped requests issued
// before any result is stored, non-temporal beyond the infinity cache); with up to twelve input streams a tile is two vectors
// per thread and stream.  When any pointer is not 16-byte aligned the whole launch goes element by element.
// StageArgs is wave_sweep_launch.hpp's StageArgsT<double>; the launcher below stays this file's own, since it refuses nothing that
// header's stage_args refuses (no stencil input, and a misaligned pointer selects the element-by-element path).
#include "wave_sweep_launch.hpp" // (StageArgs; the stages through it)

using namespace cuddh_k;
using namespace cuddh_k::wave; // the stages and fq

namespace
{
    constexpr int BLOCK = 256;
    constexpr int UNROLL = 2;
    constexpr int TILE = UNROLL * BLOCK; // 16-byte vectors per tile

    template <typename Stage, bool FORCED, bool NT>
    __global__ void __launch_bounds__(BLOCK) stage_kernel(int n, StageArgs a, int vectorised)
    {
        constexpr int NIN = Stage::NIN + (FORCED ? 2 : 0), NOUT = Stage::NOUT;
        static_assert(NIN <= MAX_IN && NOUT <= MAX_OUT, "StageArgs holds every stage");
        int done = 0;
        if (vectorised)
        {
            const int nv = n / 2;
            const int n_tiles = (nv + TILE - 1) / TILE;
            for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
            {
                const int base = tile * TILE + threadIdx.x;
                V2 x[UNROLL][NIN];
#pragma unroll
                for (int u = 0; u < UNROLL; ++u)
                {
                    const int i = min(base + u * BLOCK, nv - 1); // clamped, not guarded (blas1.hip, map_kernel)
#pragma unroll
                    for (int s = 0; s < NIN; ++s)
                        x[u][s] = stream_load<NT>(reinterpret_cast<const V2 *>(a.in[s]) + i);
                }
#pragma unroll
                for (int u = 0; u < UNROLL; ++u)
                {
                    const int i = base + u * BLOCK;
                    if (i < nv)
                    {
                        V2 y[NOUT];
#pragma unroll
                        for (int c = 0; c < 2; ++c)
                        {
                            double xe[NIN], ye[NOUT];
#pragma unroll
                            for (int s = 0; s < NIN; ++s)
                                xe[s] = x[u][s][c];
                            Stage::template apply<FORCED>(xe, ye, a.coef);
#pragma unroll
                            for (int s = 0; s < NOUT; ++s)
                                y[s][c] = ye[s];
                        }
#pragma unroll
                        for (int s = 0; s < NOUT; ++s)
                            stream_store<NT>(reinterpret_cast<V2 *>(a.out[s]) + i, y[s]);
                    }
                }
            }
            done = nv * 2;
        }
        const int tid = blockIdx.x * BLOCK + threadIdx.x, stride = gridDim.x * BLOCK;
        for (int i = done + tid; i < n; i += stride)
        {
            double xe[NIN], ye[NOUT];
#pragma unroll
            for (int s = 0; s < NIN; ++s)
                xe[s] = a.in[s][i];
            Stage::template apply<FORCED>(xe, ye, a.coef);
#pragma unroll
            for (int s = 0; s < NOUT; ++s)
                a.out[s][i] = ye[s];
        }
    }

    // in: the stage's inputs in its order; F, G: both given (forced) or both null (homogeneous)
    template <typename Stage>
    int launch_stage(int n, const double *const (&in)[Stage::NIN], const double *F, const double *G, double *const (&out)[Stage::NOUT],
                     const double (&coef)[MAX_COEF], void *stream)
    {
        if (n <= 0)
            return 0;
        if ((F == nullptr) != (G == nullptr))
            return static_cast<int>(hipErrorInvalidValue);
        const bool forced = F != nullptr;
        StageArgs a = {};
        int vec = 1;
        for (int s = 0; s < Stage::NIN; ++s)
        {
            a.in[s] = in[s];
            vec &= aligned16(in[s]);
        }
        if (forced)
        {
            a.in[Stage::NIN] = F;
            a.in[Stage::NIN + 1] = G;
            vec &= aligned16(F) && aligned16(G);
        }
        for (int s = 0; s < Stage::NOUT; ++s)
        {
            a.out[s] = out[s];
            vec &= aligned16(out[s]);
        }
        for (int s = 0; s < MAX_COEF; ++s)
            a.coef[s] = coef[s];
        long long g = (n / 2 + TILE - 1) / TILE;
        g = g < 1 ? 1 : (g > (1 << 20) ? (1 << 20) : g);
        const bool nt = static_cast<long long>(n) * sizeof(double) >= NT_BYTES;
        with_flags([&](auto forced_c, auto nt_c)
                   { hipLaunchKernelGGL((stage_kernel<Stage, decltype(forced_c)::value, decltype(nt_c)::value>), dim3(static_cast<int>(g)),
                                        dim3(BLOCK), 0, as_stream(stream), n, a, vec); },
                   forced, nt);
        return launch_status();
    }
} // namespace

extern "C"
{
    int cuddh_hip_wave_stage_begin_f64(int n, double filt0, const double *zu, const double *zv, double *p, double *q, double *u, double *v,
                                       void *stream)
    {
        return launch_stage<Begin>(n, {zu, zv}, nullptr, nullptr, {p, q, u, v}, {filt0, 0.0, 0.0, 0.0}, stream);
    }

    int cuddh_hip_wave_stage_rk2_a_f64(int n, double half_dt, double c, double s, const double *w, const double *p, const double *q,
                                       const double *invm, const double *Hi, const double *F, const double *G, double *qh, double *ph,
                                       void *stream)
    {
        return launch_stage<Rk2A>(n, {w, p, q, invm, Hi}, F, G, {qh, ph}, {half_dt, c, s, 0.0}, stream);
    }

    int cuddh_hip_wave_stage_rk2_b_f64(int n, double dt, double c, double s, double filt, const double *w, const double *qh, const double *invm,
                                       const double *Hi, const double *F, const double *G, double *p, double *q, double *u, double *v,
                                       void *stream)
    {
        return launch_stage<Rk2B>(n, {w, qh, p, q, u, v, invm, Hi}, F, G, {p, q, u, v}, {dt, c, s, filt}, stream);
    }

    int cuddh_hip_wave_stage_rk4_1_f64(int n, double half_dt, double c, double s, const double *w, const double *p, const double *q,
                                       const double *invm, const double *Hi, const double *F, const double *G, double *ps, double *qs,
                                       double *aq, double *ap, void *stream)
    {
        return launch_stage<Rk4First>(n, {w, p, q, invm, Hi}, F, G, {ps, qs, aq, ap}, {half_dt, c, s, 0.0}, stream);
    }

    int cuddh_hip_wave_stage_rk4_2_f64(int n, double half_dt, double c, double s, const double *w, const double *p, const double *q,
                                       const double *invm, const double *Hi, const double *F, const double *G, double *ps, double *qs,
                                       double *aq, double *ap, void *stream)
    {
        return launch_stage<Rk4Mid>(n, {w, p, q, qs, aq, ap, invm, Hi}, F, G, {ps, qs, aq, ap}, {half_dt, c, s, 0.0}, stream);
    }

    int cuddh_hip_wave_stage_rk4_3_f64(int n, double dt, double c, double s, const double *w, const double *p, const double *q,
                                       const double *invm, const double *Hi, const double *F, const double *G, double *ps, double *qs,
                                       double *aq, double *ap, void *stream)
    {
        return launch_stage<Rk4Mid>(n, {w, p, q, qs, aq, ap, invm, Hi}, F, G, {ps, qs, aq, ap}, {dt, c, s, 0.0}, stream);
    }

    int cuddh_hip_wave_stage_rk4_4_f64(int n, double sixth_dt, double c, double s, double filt, const double *w, const double *qs,
                                       const double *aq, const double *ap, const double *invm, const double *Hi, const double *F,
                                       const double *G, double *p, double *q, double *u, double *v, void *stream)
    {
        return launch_stage<Rk4Last>(n, {w, p, q, qs, aq, ap, u, v, invm, Hi}, F, G, {p, q, u, v}, {sixth_dt, c, s, filt}, stream);
    }
}
