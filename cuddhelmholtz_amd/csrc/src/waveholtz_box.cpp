// Whole-domain WaveHoltz on a box of brick elements (cuddh/waveholtz_box.hpp): set-up on the host (cuddh/wave_box.hpp), the march
// as the kernels of csrc/kernels/wave_box.hip (cuddh_hip_wave_box_*), one launch per sweep on padded lattice-ordered vectors.  The
// schedule is the per-sweep one of the lattice form in waveholtz.cpp; a period goes in and out through that form's gathers.
#include "cuddh/waveholtz_box.hpp"

#include <algorithm>
#include <cmath>

#include "cuddh/blas1.hpp"
#include "cuddh/launch.hpp"
#include "cuddh/time_grid.hpp"
#include "cuddh_hip.h"

namespace cuddh
{
    namespace
    {
        /// what can be refused without the box: the integrator (DDHIntegrator's rules), the ratio and omega
        void check_options(const WaveHoltzBoxOptions &o, double omega)
        {
            const DDHIntegrator &i = o.integrator;
            if (i.scheme != DDHIntegrator::rk2 && i.scheme != DDHIntegrator::rk4)
                cuddh_error("WaveHoltz error: integrator: the scheme must be rk2 or rk4.");
            if (i.coarsen < 1 || i.coarsen > DDHIntegrator::max_coarsen)
                cuddh_error(("WaveHoltz error: integrator: coarsen = " + std::to_string(i.coarsen) + " is outside [1, " +
                             std::to_string(DDHIntegrator::max_coarsen) + "].").c_str());
            if (i.scheme == DDHIntegrator::rk2 && i.coarsen != 1)
                cuddh_error("WaveHoltz error: integrator: rk2 marches on the mesh grid (coarsen = 1) only; a coarser grid needs rk4.");
            if (o.time_ratio != WaveHoltzBoxOptions::from_coefficient && (o.time_ratio < 1 || o.time_ratio > DDHTimeStep::max_ratio))
                cuddh_error(("WaveHoltz error: time step: ratio " + std::to_string(o.time_ratio) + " is outside [1, " +
                             std::to_string(DDHTimeStep::max_ratio) + "].").c_str());
            if (!std::isfinite(omega) || !(omega > 0.0))
                cuddh_error("WaveHoltz error: omega must be finite and positive.");
        }

    } // namespace

    WaveBoxTimeGrid wave_box_time_grid(double omega, int nx, int ny, int nz, const double *box, int n_basis, const double *h_a,
                                       const WaveHoltzBoxOptions &o)
    {
        check_options(o, omega);
        const double a_min = check_wave_box(nx, ny, nz, box, n_basis, h_a, o.faces);
        int ratio = o.time_ratio;
        if (ratio == WaveHoltzBoxOptions::from_coefficient)
        {
            if (std::ceil((1.0 / a_min) * (1.0 - 1e-9)) > DDHTimeStep::max_ratio)
                cuddh_error(("WaveHoltz error: time step: min a = " + std::to_string(a_min) + " asks for more than " +
                             std::to_string(DDHTimeStep::max_ratio) + " times the mesh grid's steps.").c_str());
            ratio = detail::ratio_from_coefficient(a_min);
        }
        const double min_h = std::min((box[1] - box[0]) / nx, std::min((box[3] - box[2]) / ny, (box[5] - box[4]) / nz));
        const long long steps = static_cast<long long>(ratio) * detail::coarsened_steps(detail::mesh_grid_steps(omega, min_h, n_basis), o.integrator.coarsen);
        if (steps > 0x3fffffffLL)
            cuddh_error("WaveHoltz error: time step: the period has more steps than an int holds.");
        const int nt = static_cast<int>(steps);
        return {nt, ratio, 2.0 * M_PI / omega / nt};
    }

    WaveHoltzBox::WaveHoltzBox(double omega_, int nx, int ny, int nz, const double *box, int n_basis, const double *h_a, const WaveHoltzBoxOptions &o)
        : omega(omega_), scheme(o.integrator)
    {
        // everything that is refused, before anything is allocated
        const WaveBoxTimeGrid grid = wave_box_time_grid(omega, nx, ny, nz, box, n_basis, h_a, o);
        geo = build_wave_box(nx, ny, nz, box, n_basis, h_a, o.faces);
        ndof = geo.nodes();
        slots = geo.slots();

        // ---- the period's grid
        nt = grid.nt;
        ratio = grid.ratio;
        dt = grid.dt;
        filt.resize(nt + 1);
        cs.resize(2 * nt + 1);
        sn.resize(2 * nt + 1);
        detail::fill_time_grid(omega, nt, dt, filt.data(), cs.data(), sn.data());

        // ---- maps, invm and Hi in padded lattice order (zero in the padding)
        dof_of_slot.resize(slots);
        slot_of_dof.resize(ndof);
        std::copy(geo.dof_of_slot.begin(), geo.dof_of_slot.end(), dof_of_slot.host_write());
        std::copy(geo.slot_of_dof.begin(), geo.slot_of_dof.end(), slot_of_dof.host_write());
        invm.resize(slots);
        Hi.resize(slots);
        {
            double *im = invm.host_write(), *hi = Hi.host_write();
            std::fill(im, im + slots, 0.0);
            std::fill(hi, hi + slots, 0.0);
            for (int g = 0; g < ndof; ++g)
            {
                im[geo.slot_of_dof[g]] = geo.invm[g];
                hi[geo.slot_of_dof[g]] = geo.Hi[g];
            }
        }
        invm.device_read();
        Hi.device_read();
        dof_of_slot.device_read();
        slot_of_dof.device_read();

        const bool rk4 = scheme.scheme == DDHIntegrator::rk4;
        for (host_device_dvec *x : {&p, &q, &u, &v, &ps, &qs})
            x->resize(slots);
        if (rk4)
            for (host_device_dvec *x : {&ps2, &aq, &ap})
                x->resize(slots);
        tmp.resize(2 * ndof);
    }

    WaveHoltzBox::~WaveHoltzBox() = default;

    void WaveHoltzBox::lattice(int dims[3]) const
    {
        dims[0] = geo.Lx;
        dims[1] = geo.Ly;
        dims[2] = geo.Lz;
    }

    std::string WaveHoltzBox::stiffness_kernel() const
    {
        const int nb = geo.desc.n_basis;
        return "wave_box nb" + std::to_string(nb) + (nb == 4 ? "" : " (run-time n_basis)");
    }

    void WaveHoltzBox::period(const double *z_in, const double *f, double *z_out) const
    {
        const char *what = "WaveHoltzBox::period";
        const int n = slots;
        const cuddh_wave_box *D = &geo.desc;
        void *st = stream();
        const int *dos = dof_of_slot.device_read(), *sod = slot_of_dof.device_read();
        double *P = p.device_write(), *Q = q.device_write(), *U = u.device_write(), *V = v.device_write();
        double *PS = ps.device_write(), *QS = qs.device_write();
        const double *IM = invm.device_read(), *HI = Hi.device_read(), *Ff = nullptr, *Gf = nullptr;
        if (f)
        {
            if (F.size() != n)
            {
                F.resize(n);
                G.resize(n);
            }
            double *dF = F.device_write(), *dG = G.device_write();
            detail::check_hip(cuddh_hip_wave_lattice_gather_f64(n, dos, f, dF, st), what);
            detail::check_hip(cuddh_hip_wave_lattice_gather_f64(n, dos, f + ndof, dG, st), what);
            Ff = dF;
            Gf = dG;
        }
        if (z_in)
            detail::check_hip(cuddh_hip_wave_lattice_begin_f64(n, filt[0], dos, z_in, z_in + ndof, P, Q, U, V, st), what);
        else
            for (double *y : {P, Q, U, V})
                zeros(n, y);

        if (scheme.scheme == DDHIntegrator::rk2)
        {
            for (int it = 1; it <= nt; ++it)
            {
                detail::check_hip(cuddh_hip_wave_box_rk2_a_f64(D, 0.5 * dt, cs[2 * it - 2], sn[2 * it - 2], P, Q, IM, HI, Ff, Gf, QS, PS, st), what);
                detail::check_hip(cuddh_hip_wave_box_rk2_b_f64(D, dt, cs[2 * it - 1], sn[2 * it - 1], filt[it], PS, QS, IM, HI, Ff, Gf, P, Q, U, V, st), what);
            }
        }
        else
        {
            double *AQ = aq.device_write(), *AP = ap.device_write(), *PS2 = ps2.device_write();
            for (int it = 1; it <= nt; ++it)
            {
                const int k = 2 * it - 2;
                detail::check_hip(cuddh_hip_wave_box_rk4_1_f64(D, 0.5 * dt, cs[k], sn[k], P, Q, IM, HI, Ff, Gf, PS, QS, AQ, AP, st), what);
                detail::check_hip(cuddh_hip_wave_box_rk4_2_f64(D, 0.5 * dt, cs[k + 1], sn[k + 1], PS, P, Q, IM, HI, Ff, Gf, PS2, QS, AQ, AP, st), what);
                detail::check_hip(cuddh_hip_wave_box_rk4_3_f64(D, dt, cs[k + 1], sn[k + 1], PS2, P, Q, IM, HI, Ff, Gf, PS, QS, AQ, AP, st), what);
                detail::check_hip(cuddh_hip_wave_box_rk4_4_f64(D, dt / 6.0, cs[k + 2], sn[k + 2], filt[it], PS, QS, AQ, AP, IM, HI, Ff, Gf, P, Q, U, V, st), what);
            }
        }
        detail::check_hip(cuddh_hip_gather_f64(ndof, sod, U, z_out, st), what);
        detail::check_hip(cuddh_hip_gather_f64(ndof, sod, V, z_out + ndof, st), what);
    }

    void WaveHoltzBox::solution(const double *z, double *out) const
    {
        if (out != z)
            copy(2 * ndof, z, out);
        scal(ndof, 1.0 / omega, out + ndof);
    }

    void WaveHoltzBox::action(const double *x, double *y) const
    {
        period(x, nullptr, y);
        axpby(2 * ndof, 1.0, x, -1.0, y);
    }

    void WaveHoltzBox::action(double c, const double *x, double *y) const
    {
        double *t = tmp.device_write();
        period(x, nullptr, t);
        axpby(2 * ndof, c, x, 1.0, y);
        axpby(2 * ndof, -c, t, 1.0, y);
    }
} // namespace cuddh
