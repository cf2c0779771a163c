// The per-sweep march of the lattice forms of WaveHoltz, written once (internal to waveholtz.cpp and waveholtz_box.cpp): the rk2
// and the rk4 sweep loop over one family's six entry points (cuddh_hip_wave_*_rk2_a .. _rk4_4).  The families
// differ in the arguments that lead every call: (lattice), (lattice, cell), (lattice, weight) or (box).
#ifndef CUDDH_SRC_WAVE_MARCH_HPP
#define CUDDH_SRC_WAVE_MARCH_HPP

#include "cuddh/error.hpp"

namespace cuddh
{
    namespace detail
    {
        /// the six entry points of one per-sweep kernel family
        template <auto RK2_A, auto RK2_B, auto RK4_1, auto RK4_2, auto RK4_3, auto RK4_4>
        struct SweepSet
        {
            static constexpr auto rk2_a = RK2_A, rk2_b = RK2_B, rk4_1 = RK4_1, rk4_2 = RK4_2, rk4_3 = RK4_3, rk4_4 = RK4_4;
        };

        /// the lattice vectors of one period (DEVICE); F, G null without a load; PS2, AQ, AP used by rk4 only
        template <typename R>
        struct SweepVectors
        {
            R *P, *Q, *U, *V, *PS, *QS, *PS2, *AQ, *AP, *F, *G;
            const R *IM, *HI;
        };

        /// nt steps of two sweeps.  Grid: nt, dt, filt, cs, sn (HOST) and stream; F, G: the load in lattice order, or null; `lead`:
        /// the family's leading arguments.
        template <typename Set, typename Grid, typename R, typename... Lead>
        void rk2_sweeps(const Grid &g, const SweepVectors<R> &x, const R *F, const R *G, const char *what, Lead... lead)
        {
            const double dt = g.dt, *filt = g.filt, *cs = g.cs, *sn = g.sn;
            void *st = g.stream;
            for (int it = 1; it <= g.nt; ++it)
            {
                check_hip(Set::rk2_a(lead..., 0.5 * dt, cs[2 * it - 2], sn[2 * it - 2], x.P, x.Q, x.IM, x.HI, F, G, x.QS, x.PS, st), what);
                check_hip(Set::rk2_b(lead..., dt, cs[2 * it - 1], sn[2 * it - 1], filt[it], x.PS, x.QS, x.IM, x.HI, F, G, x.P, x.Q, x.U, x.V, st), what);
            }
        }

        /// nt steps of four sweeps; rk4_2 and rk4_3 read the stencil of one ps and write the other
        template <typename Set, typename Grid, typename R, typename... Lead>
        void rk4_sweeps(const Grid &g, const SweepVectors<R> &x, const R *F, const R *G, const char *what, Lead... lead)
        {
            const double dt = g.dt, *filt = g.filt, *cs = g.cs, *sn = g.sn;
            void *st = g.stream;
            for (int it = 1; it <= g.nt; ++it)
            {
                const int k = 2 * it - 2;
                check_hip(Set::rk4_1(lead..., 0.5 * dt, cs[k], sn[k], x.P, x.Q, x.IM, x.HI, F, G, x.PS, x.QS, x.AQ, x.AP, st), what);
                check_hip(Set::rk4_2(lead..., 0.5 * dt, cs[k + 1], sn[k + 1], x.PS, x.P, x.Q, x.IM, x.HI, F, G, x.PS2, x.QS, x.AQ, x.AP, st), what);
                check_hip(Set::rk4_3(lead..., dt, cs[k + 1], sn[k + 1], x.PS2, x.P, x.Q, x.IM, x.HI, F, G, x.PS, x.QS, x.AQ, x.AP, st), what);
                check_hip(Set::rk4_4(lead..., dt / 6.0, cs[k + 2], sn[k + 2], filt[it], x.PS, x.QS, x.AQ, x.AP, x.IM, x.HI, F, G, x.P, x.Q, x.U, x.V, st), what);
            }
        }

        /// one period's sweeps on a family
        template <typename Set, typename Grid, typename R, typename... Lead>
        void sweeps(const Grid &g, const SweepVectors<R> &x, const R *F, const R *G, const char *what, Lead... lead)
        {
            if (g.rk4)
                rk4_sweeps<Set>(g, x, F, G, what, lead...);
            else
                rk2_sweeps<Set>(g, x, F, G, what, lead...);
        }
    } // namespace detail
} // namespace cuddh

#endif
