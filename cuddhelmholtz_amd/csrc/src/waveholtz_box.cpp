// Whole-domain WaveHoltz on a box of brick elements (cuddh/waveholtz_box.hpp): set-up on the host (cuddh/wave_box.hpp), the march
// as the kernels of csrc/kernels/wave_box.hip (cuddh_hip_wave_box_*), one launch per sweep on padded lattice-ordered vectors.  The
// schedule is the per-sweep one of the lattice form in waveholtz.cpp; a period goes in and out through that form's gathers.
// With precision = f32 the same call sequence on csrc/kernels/wave_box_f32.hip (cuddh_hip_wave_box32_*), in and out through
// cuddh_hip_wave32_load / _begin / _store.
// The per-sweep loops are wave_march.hpp's, shared with waveholtz.cpp.
#include "cuddh/waveholtz_box.hpp"

#include <algorithm>
#include <cmath>

#include "cuddh/blas1.hpp"
#include "cuddh/launch.hpp"
#include "cuddh/time_grid.hpp"
#include "cuddh_hip.h"
#include "wave_march.hpp"

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
            if (o.precision != WaveHoltzBoxOptions::f64 && o.precision != WaveHoltzBoxOptions::f32)
                cuddh_error("WaveHoltz error: precision: the precision must be f64 or f32.");
        }

        /// rows of the fp32 sweeps hold a multiple of four floats (16 bytes), those of the fp64 sweeps of two doubles
        int row_multiple(const WaveHoltzBoxOptions &o) { return o.precision == WaveHoltzBoxOptions::f32 ? 4 : 2; }

        /// The two kernel families behind one set of names: R = double is cuddh_hip_wave_box_*_f64 between the lattice form's
        /// fp64 gathers, R = float is cuddh_hip_wave_box32_* between cuddh_hip_wave32_load / _begin / _store.  `sweeps` is the
        /// per-sweep family that wave_march.hpp marches on; its calls lead with (box).
        template <typename R>
        struct BoxKernels;
        template <>
        struct BoxKernels<double>
        {
            static constexpr auto load = cuddh_hip_wave_lattice_gather_f64;
            static constexpr auto store = cuddh_hip_gather_f64;
            static constexpr auto begin = cuddh_hip_wave_lattice_begin_f64;
            using sweeps = detail::SweepSet<cuddh_hip_wave_box_rk2_a_f64, cuddh_hip_wave_box_rk2_b_f64, cuddh_hip_wave_box_rk4_1_f64,
                                            cuddh_hip_wave_box_rk4_2_f64, cuddh_hip_wave_box_rk4_3_f64, cuddh_hip_wave_box_rk4_4_f64>;
        };
        template <>
        struct BoxKernels<float>
        {
            static constexpr auto load = cuddh_hip_wave32_load;
            static constexpr auto store = cuddh_hip_wave32_store;
            static constexpr auto begin = cuddh_hip_wave32_begin;
            using sweeps = detail::SweepSet<cuddh_hip_wave_box32_rk2_a, cuddh_hip_wave_box32_rk2_b, cuddh_hip_wave_box32_rk4_1,
                                            cuddh_hip_wave_box32_rk4_2, cuddh_hip_wave_box32_rk4_3, cuddh_hip_wave_box32_rk4_4>;
        };

        template <typename R>
        using BoxVectors = detail::SweepVectors<R>; // the lattice vectors of one period (wave_march.hpp)

        /// what a period reads besides its vectors
        struct BoxGrid
        {
            const cuddh_wave_box *D;
            int slots, ndof, nt;
            bool rk4;
            double dt;
            const double *filt, *cs, *sn; // HOST
            const int *dof_of_slot, *slot_of_dof;
            void *stream;
        };

        template <typename R>
        void box_march(const BoxGrid &g, const BoxVectors<R> &x, const double *z_in, const double *f, double *z_out)
        {
            using Kn = BoxKernels<R>;
            const char *what = "WaveHoltzBox::period";
            const int n = g.slots, ndof = g.ndof;
            void *st = g.stream;
            R *P = x.P, *Q = x.Q, *U = x.U, *V = x.V;
            const R *Ff = nullptr, *Gf = nullptr;
            if (f)
            {
                detail::check_hip(Kn::load(n, g.dof_of_slot, f, x.F, st), what);
                detail::check_hip(Kn::load(n, g.dof_of_slot, f + ndof, x.G, st), what);
                Ff = x.F;
                Gf = x.G;
            }
            if (z_in)
                detail::check_hip(Kn::begin(n, g.filt[0], g.dof_of_slot, z_in, z_in + ndof, P, Q, U, V, st), what);
            else
                for (R *y : {P, Q, U, V})
                    zeros(n, y);

            detail::sweeps<typename Kn::sweeps>(g, x, Ff, Gf, what, g.D);
            detail::check_hip(Kn::store(ndof, g.slot_of_dof, U, z_out, st), what);
            detail::check_hip(Kn::store(ndof, g.slot_of_dof, V, z_out + ndof, st), what);
        }
    } // namespace

    WaveBoxTimeGrid wave_box_time_grid(double omega, int nx, int ny, int nz, const double *box, int n_basis, const double *h_a,
                                       const WaveHoltzBoxOptions &o)
    {
        check_options(o, omega);
        const double a_min = check_wave_box(nx, ny, nz, box, n_basis, h_a, o.faces, row_multiple(o));
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
        : omega(omega_), scheme(o.integrator), f32(o.precision == WaveHoltzBoxOptions::f32)
    {
        // everything that is refused, before anything is allocated
        const WaveBoxTimeGrid grid = wave_box_time_grid(omega, nx, ny, nz, box, n_basis, h_a, o);
        geo = build_wave_box(nx, ny, nz, box, n_basis, h_a, o.faces, row_multiple(o));
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
        const bool rk4 = scheme.scheme == DDHIntegrator::rk4;
        if (f32)
        {
            // invm and Hi, formed in double, into lattice order as floats, each rounded once; the padding slots get zero.  The
            // class's double lattice vectors are not allocated.
            const int *dos = dof_of_slot.device_read();
            slot_of_dof.device_read();
            invm32.resize(slots);
            Hi32.resize(slots);
            host_device_dvec t(ndof);
            for (const auto &x : {std::make_pair(&geo.invm, &invm32), std::make_pair(&geo.Hi, &Hi32)})
            {
                std::copy(x.first->begin(), x.first->end(), t.host_write());
                detail::check_hip(cuddh_hip_wave32_load(slots, dos, t.device_read(), x.second->device_write(), stream()), "WaveHoltzBox lattice order");
                detail::check_hip(cuddh_hip_stream_sync(stream()), "WaveHoltzBox setup"); // t is overwritten, then dies
            }
            for (HostDeviceArray<float> *x : {&p32, &q32, &u32, &v32, &ps32, &qs32})
                x->resize(slots);
            if (rk4)
                for (HostDeviceArray<float> *x : {&ps2_32, &aq32, &ap32})
                    x->resize(slots);
            tmp.resize(2 * ndof);
            return;
        }
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
        if (f32)
            return "wave_box nb" + std::to_string(nb) + " f32" + (nb == 4 || nb == 5 ? "" : " (run-time n_basis)");
        return "wave_box nb" + std::to_string(nb) + (nb == 4 ? "" : " (run-time n_basis)");
    }

    void WaveHoltzBox::period(const double *z_in, const double *f, double *z_out) const
    {
        const int n = slots;
        const bool rk4 = scheme.scheme == DDHIntegrator::rk4;
        const BoxGrid g = {&geo.desc, n, ndof, nt, rk4, dt, filt.data(), cs.data(), sn.data(), dof_of_slot.device_read(), slot_of_dof.device_read(), stream()};
        if (f32)
        {
            if (f && F32.size() != n)
            {
                F32.resize(n);
                G32.resize(n);
            }
            const BoxVectors<float> x = {p32.device_write(), q32.device_write(), u32.device_write(), v32.device_write(), ps32.device_write(),
                                         qs32.device_write(), rk4 ? ps2_32.device_write() : nullptr, rk4 ? aq32.device_write() : nullptr,
                                         rk4 ? ap32.device_write() : nullptr, f ? F32.device_write() : nullptr, f ? G32.device_write() : nullptr,
                                         invm32.device_read(), Hi32.device_read()};
            return box_march(g, x, z_in, f, z_out);
        }
        if (f && F.size() != n)
        {
            F.resize(n);
            G.resize(n);
        }
        const BoxVectors<double> x = {p.device_write(), q.device_write(), u.device_write(), v.device_write(), ps.device_write(),
                                      qs.device_write(), rk4 ? ps2.device_write() : nullptr, rk4 ? aq.device_write() : nullptr,
                                      rk4 ? ap.device_write() : nullptr, f ? F.device_write() : nullptr, f ? G.device_write() : nullptr,
                                      invm.device_read(), Hi.device_read()};
        box_march(g, x, z_in, f, z_out);
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
