// What the two paired-sweep files share (wave_pair.hip: fp64; wave_pair_f32.hip: fp32): two consecutive sweeps of
// the lattice march composed into one launch.  In both integrators the stencil input of the second sweep of a pair is pointwise
// in vectors that exist before the first one runs:
//   rk2     (rk2_a, rk2_b):   K p   and  K ph,   ph  = fma(-dt/2, q, p)
//   rk4_12  (rk4_1, rk4_2):   K p   and  K ps1,  ps1 = fma(-dt/2, q, p)
//   rk4_34  (rk4_3, rk4_4):   K ps2 and  K ps3,  ps3 = fma(-dt, qs, p),   qs the vector rk4_2 wrote
// so a workgroup stages two tiles, one stored and one derived while staging, evaluates two stencils and runs the two stages of
// wave_stages.hpp back to back with the first stage's outputs in registers.  A pair is its two stages called in the march's order
// on the march's values: every operation is the fused multiply-add the one-sweep kernels do, in their order, and the results
// are theirs bit for bit.
#ifndef CUDDH_AMD_WAVE_PAIR_STAGES_HPP
#define CUDDH_AMD_WAVE_PAIR_STAGES_HPP

#include "wave_lattice_common.hpp"
#include "wave_sweep_launch.hpp" // (dispatch_sweep and invalid_value for the two launchers; the stages through it)

namespace cuddh_k
{
    namespace wave
    {
        constexpr int PAIR_HALO = 3, PAIR_MAX_IN = 11, PAIR_MAX_OUT = 4, PAIR_MAX_COEF = 7;

        template <typename R>
        struct PairArgsT
        {
            // read with a halo: tile 1 is halo[0]; tile 2 is fma(-coef[0], halo[2], halo[1])  (halo[1] == halo[0] when P_IS_TILE)
            const R *halo[PAIR_HALO];
            const R *in[PAIR_MAX_IN]; // the pointwise streams, (F, G) behind them when forced
            R *out[PAIR_MAX_OUT];     // may alias `in` (element i is read before it is written, by the same thread), never `halo`
            R coef[PAIR_MAX_COEF];    // coef[0]: the step of the derived tile
        };

        // A pair: NIN streams besides (F, G), NOUT outputs; apply() on one node, wa = (K tile 1), wb = (K tile 2), p = tile 1 there.
        template <typename R>
        struct PairRk2T
        {
            static constexpr int NIN = 5, NOUT = 4; // in: q u v invm Hi; out: p q u v; coef: dt/2 dt c0 s0 c1 s1 filt
            static constexpr bool P_IS_TILE = true; // halo: p q
            static constexpr bool halo_stream(int s) { return s == 0; }
            template <bool FORCED>
            __device__ static void apply(R wa, R wb, R p, const R *s, R *y, const R *k)
            {
                using A = Rk2AT<R>;
                using B = Rk2BT<R>;
                R xa[A::NIN + 2] = {wa, p, s[0], s[3], s[4]}, ya[A::NOUT];
                R xb[B::NIN + 2] = {wb, R(0), p, s[0], s[1], s[2], s[3], s[4]};
                if constexpr (FORCED)
                {
                    xa[A::NIN] = xb[B::NIN] = s[NIN];
                    xa[A::NIN + 1] = xb[B::NIN + 1] = s[NIN + 1];
                }
                const R ka[3] = {k[0], k[2], k[3]}, kb[4] = {k[1], k[4], k[5], k[6]};
                A::template apply<FORCED>(xa, ya, ka);
                xb[1] = ya[0]; // qh
                B::template apply<FORCED>(xb, y, kb);
            }
        };
        template <typename R>
        struct PairRk4_12T
        {
            static constexpr int NIN = 3, NOUT = 4; // in: q invm Hi; out: ps2 qs aq ap; coef: dt/2 c0 s0 c1 s1
            static constexpr bool P_IS_TILE = true; // halo: p q
            static constexpr bool halo_stream(int s) { return s == 0; }
            template <bool FORCED>
            __device__ static void apply(R wa, R wb, R p, const R *s, R *y, const R *k)
            {
                using A = Rk4FirstT<R>;
                using B = Rk4MidT<R>;
                R xa[A::NIN + 2] = {wa, p, s[0], s[1], s[2]}, ya[A::NOUT];
                R xb[B::NIN + 2] = {wb, p, s[0], R(0), R(0), R(0), s[1], s[2]};
                if constexpr (FORCED)
                {
                    xa[A::NIN] = xb[B::NIN] = s[NIN];
                    xa[A::NIN + 1] = xb[B::NIN + 1] = s[NIN + 1];
                }
                const R ka[3] = {k[0], k[1], k[2]}, kb[3] = {k[0], k[3], k[4]};
                A::template apply<FORCED>(xa, ya, ka);
                xb[3] = ya[1]; // qs, aq, ap of rk4_1 (its ps is tile 2)
                xb[4] = ya[2];
                xb[5] = ya[3];
                B::template apply<FORCED>(xb, y, kb);
            }
        };
        template <typename R>
        struct PairRk4_34T
        {
            static constexpr int NIN = 9, NOUT = 4;  // in: p q qs aq ap u v invm Hi; out: p q u v; coef: dt dt/6 c1 s1 c2 s2 filt
            static constexpr bool P_IS_TILE = false; // halo: ps2 p qs
            static constexpr bool halo_stream(int s) { return s == 0 || s == 2; }
            template <bool FORCED>
            __device__ static void apply(R wa, R wb, R, const R *s, R *y, const R *k)
            {
                using A = Rk4MidT<R>;
                using B = Rk4LastT<R>;
                R xa[A::NIN + 2] = {wa, s[0], s[1], s[2], s[3], s[4], s[7], s[8]}, ya[A::NOUT];
                R xb[B::NIN + 2] = {wb, s[0], s[1], R(0), R(0), R(0), s[5], s[6], s[7], s[8]};
                if constexpr (FORCED)
                {
                    xa[A::NIN] = xb[B::NIN] = s[NIN];
                    xa[A::NIN + 1] = xb[B::NIN + 1] = s[NIN + 1];
                }
                const R ka[3] = {k[0], k[2], k[3]}, kb[4] = {k[1], k[4], k[5], k[6]};
                A::template apply<FORCED>(xa, ya, ka);
                xb[3] = ya[1]; // qs, aq, ap of rk4_3 (its ps is tile 2)
                xb[4] = ya[2];
                xb[5] = ya[3];
                B::template apply<FORCED>(xb, y, kb);
            }
        };

        // The kernel's arguments from the caller's, or false: a bad description, F / G given singly, a NULL or misaligned pointer,
        // or an output that is read with a halo (a neighbouring workgroup still needs it).  coef is rounded to R here, once.
        template <typename R, typename Kind, int NCOEF>
        bool pair_args(const cuddh_wave_lattice *D, int stride_multiple, const R *const (&halo)[PAIR_HALO], const R *const (&in)[Kind::NIN],
                       const R *F, const R *G, R *const (&out)[Kind::NOUT], const double (&coef)[NCOEF], LatticeT<R> &L, PairArgsT<R> &a)
        {
            static_assert(NCOEF <= PAIR_MAX_COEF && Kind::NIN + 2 <= PAIR_MAX_IN && Kind::NOUT <= PAIR_MAX_OUT, "PairArgsT holds every pair");
            if (!describe(D, stride_multiple, L) || (F == nullptr) != (G == nullptr))
                return false;
            a = {};
            bool ok = true;
            for (int h = 0; h < PAIR_HALO; ++h)
            {
                a.halo[h] = halo[h];
                ok = ok && halo[h] && aligned16(halo[h]);
            }
            for (int s = 0; s < Kind::NIN; ++s)
            {
                a.in[s] = in[s];
                ok = ok && in[s] && aligned16(in[s]);
            }
            if (F)
            {
                a.in[Kind::NIN] = F;
                a.in[Kind::NIN + 1] = G;
                ok = ok && aligned16(F) && aligned16(G);
            }
            for (int s = 0; s < Kind::NOUT; ++s)
            {
                a.out[s] = out[s];
                ok = ok && out[s] && aligned16(out[s]);
                for (int h = 0; h < PAIR_HALO; ++h)
                    ok = ok && out[s] != halo[h];
            }
            for (int s = 0; s < NCOEF; ++s)
                a.coef[s] = static_cast<R>(coef[s]);
            return ok;
        }
    } // namespace wave
} // namespace cuddh_k

#endif
