// The WaveHoltz time grid: one period T = 2 pi / omega in nt steps, and the tables a march over it reads.  Shared by the DDH
// local solves (src/ddh.cpp) and the whole-domain march (src/waveholtz.cpp), so that both step on the same grids.
#ifndef CUDDH_AMD_TIME_GRID_HPP
#define CUDDH_AMD_TIME_GRID_HPP

#include <algorithm>
#include <cmath>

namespace cuddh
{
    namespace detail
    {
        /// steps of the mesh grid: dt = 0.1 h / n_basis^2 shrunk so that nt dt is one period (reference source/DDH.cpp)
        inline int mesh_grid_steps(double omega, double min_h, int n_basis)
        {
            const double T = 2.0 * M_PI / omega;
            const double dt = 0.2 * 0.5 * min_h / (n_basis * n_basis);
            return static_cast<int>(std::ceil(T / dt));
        }

        /// steps of the base grid of an integrator that coarsens the mesh grid: ceil(nt_mesh / coarsen)
        inline int coarsened_steps(int nt_mesh, int coarsen) { return (nt_mesh + coarsen - 1) / coarsen; }

        /// the time ratio the coefficient asks for: the wave speed is 1 / a.  (1 - 1e-9) keeps 1 / a that is an integer up to
        /// rounding (a = 0.2) on that integer
        inline int ratio_from_coefficient(double a_min) { return std::max(1, static_cast<int>(std::ceil((1.0 / a_min) * (1.0 - 1e-9)))); }

        /// WaveHoltz tables of the grid of nt steps of dt = T / nt: filter (nt + 1: trapezoid weights of the period
        /// average), cs and sn (2 nt + 1: -cos and sin at the half steps); computed in double, rounded to Real
        template <typename Real>
        void fill_time_grid(double omega, int nt, double dt, Real *filt, Real *cs, Real *sn)
        {
            for (int k = 0; k <= nt; ++k)
                filt[k] = static_cast<Real>(dt * (omega / M_PI) * (std::cos(omega * k * dt) - 0.25));
            filt[0] = static_cast<Real>(filt[0] * 0.5); // trapezoid rule end points
            filt[nt] = static_cast<Real>(filt[nt] * 0.5);
            for (int k = 0; k <= 2 * nt; ++k)
            {
                const double t = 0.5 * k * dt;
                cs[k] = static_cast<Real>(-std::cos(omega * t));
                sn[k] = static_cast<Real>(std::sin(omega * t));
            }
        }
    } // namespace detail
} // namespace cuddh

#endif
