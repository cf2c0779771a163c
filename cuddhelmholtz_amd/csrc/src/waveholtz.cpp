// Whole-domain WaveHoltz (cuddh/waveholtz.hpp): set-up on the host, the march as stiffness applies and the stage kernels of
// csrc/kernels/waveholtz.hip (cuddh_hip_wave_stage_*), one launch of each per sweep; or, in the lattice form, as the kernels of
// csrc/kernels/wave_lattice.hip (cuddh_hip_wave_lattice_*), one launch per sweep on lattice-ordered vectors; with precision = f32
// the same call sequence on the fp32 family of csrc/kernels/wave_lattice_f32.hip (cuddh_hip_wave32_*); with launch = per_pair two
// sweeps per launch (csrc/kernels/wave_pair.hip and wave_pair_f32.hip: cuddh_hip_wave_pair_*, cuddh_hip_wave_pair32_*); on a grid
// mesh with missing cells the per-sweep sequence on csrc/kernels/wave_cells.hip and wave_cells_f32.hip (cuddh_hip_wave_cells_*,
// cuddh_hip_wave_cells32_*); with a per-cell stiffness coefficient the per-sweep sequence on csrc/kernels/wave_weights.hip
// and wave_weights_f32.hip (cuddh_hip_wave_weights_*, cuddh_hip_wave_weights32_*).
// The per-sweep loops are written once, in wave_march.hpp, for every family and for waveholtz_box.cpp.
#include "cuddh/waveholtz.hpp"

#include <algorithm>
#include <cmath>
#include <string>
#include <utility>

#include "cuddh/time_grid.hpp"
#include "cuddh/wave_lattice.hpp"
#include "cuddh_hip.h"
#include "wave_march.hpp"

namespace cuddh
{
    namespace
    {
        /// the options that can be refused without the mesh: the integrator (DDHIntegrator's rules) and the ratio
        void check_options(const WaveHoltzOptions &o)
        {
            const DDHIntegrator &i = o.integrator;
            if (i.scheme != DDHIntegrator::rk2 && i.scheme != DDHIntegrator::rk4)
                cuddh_error("WaveHoltz error: integrator: the scheme must be rk2 or rk4.");
            if (i.coarsen < 1 || i.coarsen > DDHIntegrator::max_coarsen)
                cuddh_error(("WaveHoltz error: integrator: coarsen = " + std::to_string(i.coarsen) + " is outside [1, " +
                             std::to_string(DDHIntegrator::max_coarsen) + "].").c_str());
            if (i.scheme == DDHIntegrator::rk2 && i.coarsen != 1)
                cuddh_error("WaveHoltz error: integrator: rk2 marches on the mesh grid (coarsen = 1) only; a coarser grid needs rk4.");
            if (o.time_ratio != WaveHoltzOptions::from_coefficient && (o.time_ratio < 1 || o.time_ratio > DDHTimeStep::max_ratio))
                cuddh_error(("WaveHoltz error: time step: ratio " + std::to_string(o.time_ratio) + " is outside [1, " +
                             std::to_string(DDHTimeStep::max_ratio) + "].").c_str());
            if (o.stiffness != WaveHoltzOptions::gauss && o.stiffness != WaveHoltzOptions::lobatto)
                cuddh_error("WaveHoltz error: stiffness: the rule must be gauss or lobatto.");
            if (o.n_faces > 0 && !o.h_faces)
                cuddh_error("WaveHoltz error: faces: a list of absorbing faces was announced and none given.");
            if (o.sweep != WaveHoltzOptions::operator_kernels && o.sweep != WaveHoltzOptions::lattice)
                cuddh_error("WaveHoltz error: sweep: the form must be operator_kernels or lattice.");
            if (o.sweep == WaveHoltzOptions::lattice && o.stiffness != WaveHoltzOptions::lobatto)
                cuddh_error("WaveHoltz error: sweep: the lattice form is the collocated stiffness; it needs stiffness = lobatto.");
            if (o.precision != WaveHoltzOptions::f64 && o.precision != WaveHoltzOptions::f32)
                cuddh_error("WaveHoltz error: precision: the precision must be f64 or f32.");
            if (o.precision == WaveHoltzOptions::f32 && o.sweep != WaveHoltzOptions::lattice)
                cuddh_error("WaveHoltz error: precision: f32 is an option of the lattice form; it needs sweep = lattice.");
            if (o.launch != WaveHoltzOptions::per_sweep && o.launch != WaveHoltzOptions::per_pair)
                cuddh_error("WaveHoltz error: launch: the launch must be per_sweep or per_pair.");
            if (o.launch == WaveHoltzOptions::per_pair && o.sweep != WaveHoltzOptions::lattice)
                cuddh_error("WaveHoltz error: launch: per_pair is an option of the lattice form; it needs sweep = lattice.");
            if (o.h_cell_stiffness && o.sweep != WaveHoltzOptions::lattice)
                cuddh_error("WaveHoltz error: cell_stiffness: a per-cell stiffness is an option of the lattice form; it needs sweep = lattice.");
            if (o.h_cell_stiffness && o.launch == WaveHoltzOptions::per_pair)
                cuddh_error("WaveHoltz error: launch: per_pair has no form for a per-cell stiffness; it needs launch = per_sweep.");
        }

        host_device_dvec rule_weights(const QuadratureRule &quad)
        {
            host_device_dvec w(quad.size());
            double *h = w.host_write();
            for (int i = 0; i < quad.size(); ++i)
                h[i] = quad.w(i);
            return w;
        }

        /// The kernel families of the lattice form behind one set of names: R = double is cuddh_hip_wave_lattice_*_f64 (and
        /// cuddh_hip_gather_f64 on the way out), R = float is cuddh_hip_wave32_*.  `plain`, `cells` and `weights` are the per-sweep
        /// families that wave_march.hpp marches on; their calls lead with (lattice), (lattice, cell) and (lattice, weight).
        template <typename R>
        struct LatticeKernels;
        template <>
        struct LatticeKernels<double>
        {
            static constexpr auto load = cuddh_hip_wave_lattice_gather_f64;
            static constexpr auto store = cuddh_hip_gather_f64;
            static constexpr auto begin = cuddh_hip_wave_lattice_begin_f64;
            static constexpr auto pair_rk2 = cuddh_hip_wave_pair_rk2_f64;
            static constexpr auto pair_rk4_12 = cuddh_hip_wave_pair_rk4_12_f64;
            static constexpr auto pair_rk4_34 = cuddh_hip_wave_pair_rk4_34_f64;
            using plain = detail::SweepSet<cuddh_hip_wave_lattice_rk2_a_f64, cuddh_hip_wave_lattice_rk2_b_f64, cuddh_hip_wave_lattice_rk4_1_f64,
                                           cuddh_hip_wave_lattice_rk4_2_f64, cuddh_hip_wave_lattice_rk4_3_f64, cuddh_hip_wave_lattice_rk4_4_f64>;
            using cells = detail::SweepSet<cuddh_hip_wave_cells_rk2_a_f64, cuddh_hip_wave_cells_rk2_b_f64, cuddh_hip_wave_cells_rk4_1_f64,
                                           cuddh_hip_wave_cells_rk4_2_f64, cuddh_hip_wave_cells_rk4_3_f64, cuddh_hip_wave_cells_rk4_4_f64>;
            using weights = detail::SweepSet<cuddh_hip_wave_weights_rk2_a_f64, cuddh_hip_wave_weights_rk2_b_f64, cuddh_hip_wave_weights_rk4_1_f64,
                                             cuddh_hip_wave_weights_rk4_2_f64, cuddh_hip_wave_weights_rk4_3_f64, cuddh_hip_wave_weights_rk4_4_f64>;
        };
        template <>
        struct LatticeKernels<float>
        {
            static constexpr auto load = cuddh_hip_wave32_load;
            static constexpr auto store = cuddh_hip_wave32_store;
            static constexpr auto begin = cuddh_hip_wave32_begin;
            static constexpr auto pair_rk2 = cuddh_hip_wave_pair32_rk2;
            static constexpr auto pair_rk4_12 = cuddh_hip_wave_pair32_rk4_12;
            static constexpr auto pair_rk4_34 = cuddh_hip_wave_pair32_rk4_34;
            using plain = detail::SweepSet<cuddh_hip_wave32_rk2_a, cuddh_hip_wave32_rk2_b, cuddh_hip_wave32_rk4_1, cuddh_hip_wave32_rk4_2,
                                           cuddh_hip_wave32_rk4_3, cuddh_hip_wave32_rk4_4>;
            using cells = detail::SweepSet<cuddh_hip_wave_cells32_rk2_a, cuddh_hip_wave_cells32_rk2_b, cuddh_hip_wave_cells32_rk4_1,
                                           cuddh_hip_wave_cells32_rk4_2, cuddh_hip_wave_cells32_rk4_3, cuddh_hip_wave_cells32_rk4_4>;
            using weights = detail::SweepSet<cuddh_hip_wave_weights32_rk2_a, cuddh_hip_wave_weights32_rk2_b, cuddh_hip_wave_weights32_rk4_1,
                                             cuddh_hip_wave_weights32_rk4_2, cuddh_hip_wave_weights32_rk4_3, cuddh_hip_wave_weights32_rk4_4>;
        };

        /// the lattice vectors of one period (wave_march.hpp) and, with a per-cell stiffness, the cell weights of wave_weights.hip
        template <typename R>
        struct LatticeVectors : detail::SweepVectors<R>
        {
            const R *W = nullptr; // nx ny weights (DEVICE), null without a per-cell stiffness
        };

        /// what a period reads besides its vectors
        struct LatticeGrid
        {
            const cuddh_wave_lattice *D;
            int slots, ndof, nt;
            bool rk4, pair;
            double dt;
            const double *filt, *cs, *sn; // HOST
            const int *dof_of_slot, *slot_of_dof;
            void *stream;
            const unsigned char *cell = nullptr; // DEVICE flags of a grid with missing cells (wave_cells.hip), null on a full grid
        };

        template <typename R>
        void lattice_march(const LatticeGrid &g, const LatticeVectors<R> &x, const double *z_in, const double *f, double *z_out)
        {
            using Kn = LatticeKernels<R>;
            const int n = g.slots, ndof = g.ndof;
            const cuddh_wave_lattice *D = g.D;
            const char *what = "WaveHoltz::period (lattice)";
            void *st = g.stream;
            const double dt = g.dt, *filt = g.filt, *cs = g.cs, *sn = g.sn;
            R *P = x.P, *Q = x.Q, *U = x.U, *V = x.V, *PS = x.PS, *QS = x.QS;
            const R *IM = x.IM, *HI = x.HI, *Ff = nullptr, *Gf = nullptr;
            if (f)
            {
                detail::check_hip(Kn::load(n, g.dof_of_slot, f, x.F, st), what);
                detail::check_hip(Kn::load(n, g.dof_of_slot, f + ndof, x.G, st), what);
                Ff = x.F;
                Gf = x.G;
            }
            if (z_in)
                detail::check_hip(Kn::begin(n, filt[0], g.dof_of_slot, z_in, z_in + ndof, P, Q, U, V, st), what);
            else
                for (R *y : {P, Q, U, V})
                    zeros(n, y);

            if (g.pair && !g.rk4)
            {
                // two sweeps per launch (wave_pair.hip): p and q are read with a halo, so a step writes the other pair of buffers
                R *P2 = PS, *Q2 = QS;
                for (int it = 1; it <= g.nt; ++it)
                {
                    detail::check_hip(Kn::pair_rk2(D, 0.5 * dt, dt, cs[2 * it - 2], sn[2 * it - 2], cs[2 * it - 1], sn[2 * it - 1], filt[it], P, Q, IM,
                                                   HI, Ff, Gf, P2, Q2, U, V, st),
                                      what);
                    std::swap(P, P2);
                    std::swap(Q, Q2);
                }
            }
            else if (g.pair)
            {
                // rk4_1 with rk4_2, then rk4_3 with rk4_4; the second launch reads p with a halo and writes the other p
                R *AQ = x.AQ, *AP = x.AP, *PS2 = x.PS2, *P2 = PS;
                for (int it = 1; it <= g.nt; ++it)
                {
                    const int k = 2 * it - 2;
                    detail::check_hip(Kn::pair_rk4_12(D, 0.5 * dt, cs[k], sn[k], cs[k + 1], sn[k + 1], P, Q, IM, HI, Ff, Gf, PS2, QS, AQ, AP, st), what);
                    detail::check_hip(Kn::pair_rk4_34(D, dt, dt / 6.0, cs[k + 1], sn[k + 1], cs[k + 2], sn[k + 2], filt[it], PS2, P, QS, AQ, AP, IM, HI,
                                                      Ff, Gf, P2, Q, U, V, st),
                                      what);
                    std::swap(P, P2);
                }
            }
            else if (x.W)
                detail::sweeps<typename Kn::weights>(g, x, Ff, Gf, what, D, x.W);
            else if (g.cell)
                detail::sweeps<typename Kn::cells>(g, x, Ff, Gf, what, D, g.cell);
            else
                detail::sweeps<typename Kn::plain>(g, x, Ff, Gf, what, D);
            detail::check_hip(Kn::store(ndof, g.slot_of_dof, U, z_out, st), what);
            detail::check_hip(Kn::store(ndof, g.slot_of_dof, V, z_out + ndof, st), what);
        }
    } // namespace

    struct WaveHoltz::Lattice
    {
        cuddh_wave_lattice desc = {};
        int slots = 0;                              // elements per lattice vector: stride * Ly
        host_device_ivec dof_of_slot, slot_of_dof;  // slots (-1: padding or a node with no cell around it) and ndof
        HostDeviceArray<unsigned char> cell;        // a grid with missing cells (wave_cells.hip): nx ny flags; empty on a full grid
        mutable host_device_dvec ps2;               // rk4_2 and rk4_3 read the stencil of one ps and write the other
        // precision = f32: the thirteen lattice vectors as floats (the class's double ones then stay empty)
        bool f32 = false;
        bool pair = false;                          // launch = per_pair: two sweeps per launch (wave_pair.hip)
        HostDeviceArray<float> invm, Hi;
        mutable HostDeviceArray<float> p, q, u, v, ps, qs, ps2f, aq, ap, F, G;
        // a per-cell stiffness (wave_weights.hip): nx ny weights in the march's precision, rounded once for f32; empty without one
        host_device_dvec weight;
        HostDeviceArray<float> weight32;
        bool weighted() const { return weight.size() || weight32.size(); }
    };

    WaveHoltz::WaveHoltz(double omega_, const double *h_a, const H1Space &fem, const WaveHoltzOptions &o)
        : omega(omega_), ndof(fem.size()), scheme(o.integrator), invm(fem.size()), Hi(fem.size())
    {
        check_options(o);
        if (!std::isfinite(omega) || !(omega > 0.0))
            cuddh_error("WaveHoltz error: omega must be finite and positive.");
        double a_min = INFINITY;
        for (int g = 0; g < ndof; ++g)
        {
            if (!std::isfinite(h_a[g]) || !(h_a[g] > 0.0))
                cuddh_error(("WaveHoltz error: a = " + std::to_string(h_a[g]) + " at dof " + std::to_string(g) + "; a must be finite and positive.").c_str());
            a_min = std::min(a_min, h_a[g]);
        }
        if (o.h_cell_stiffness)
            check_cell_stiffness(fem.mesh().n_elem(), o.h_cell_stiffness);
        ratio = o.time_ratio;
        if (ratio == WaveHoltzOptions::from_coefficient && o.h_cell_stiffness)
        {
            const int nb1 = fem.basis().size();
            ratio = wave_coefficient_ratio(fem.mesh().n_elem(), nb1 * nb1, fem.global_indices(MemorySpace::HOST), h_a, o.h_cell_stiffness);
        }
        else if (ratio == WaveHoltzOptions::from_coefficient)
        {
            if (std::ceil((1.0 / a_min) * (1.0 - 1e-9)) > DDHTimeStep::max_ratio)
                cuddh_error(("WaveHoltz error: time step: min a = " + std::to_string(a_min) + " asks for more than " +
                             std::to_string(DDHTimeStep::max_ratio) + " times the mesh grid's steps.").c_str());
            ratio = detail::ratio_from_coefficient(a_min);
        }

        // ---- the lattice form: the mesh is detected (and refused) before anything is allocated
        if (o.sweep == WaveHoltzOptions::lattice)
        {
            if (fem.basis().size() > 8)
                cuddh_error("WaveHoltz error: sweep: the lattice kernels take n_basis up to 8.");
            // a full grid runs wave_lattice.hip; only where that detection refuses is a grid with missing cells looked for
            const WaveLatticeMap map = build_wave_lattice_or_cells_map(fem);
            if (!map.cell.empty() && o.launch == WaveHoltzOptions::per_pair)
                cuddh_error("WaveHoltz error: launch: per_pair needs a full uniform rectangle mesh; the paired kernels have no form for a grid "
                            "with missing cells yet.");
            // rows of the fp32 form hold a multiple of four floats (16 bytes), those of the fp64 form the map's even stride
            const bool f32 = o.precision == WaveHoltzOptions::f32;
            const int stride = f32 ? (map.Lx + 3) / 4 * 4 : map.stride;
            if (static_cast<long long>(stride) * map.Ly > 0x7fffffffLL)
                cuddh_error("WaveHoltz error: precision: the padded fp32 lattice does not fit in an int.");
            lat.reset(new Lattice);
            lat->f32 = f32;
            lat->pair = o.launch == WaveHoltzOptions::per_pair;
            lat->desc.nx = map.nx;
            lat->desc.ny = map.ny;
            lat->desc.n_basis = map.n_basis;
            lat->desc.stride = stride;
            lat->desc.cx = map.hy / map.hx;
            lat->desc.cy = map.hx / map.hy;
            wave_lattice_tables(fem.basis(), lat->desc.A, lat->desc.w);
            if (o.h_cell_stiffness)
            {
                // the weighted kernels take full and holed grids alike: an absent cell is weight zero, and no flags are kept
                const std::vector<double> wts = wave_lattice_cell_weights(map, fem.mesh().n_elem(), o.h_cell_stiffness);
                const int n_cells = static_cast<int>(wts.size());
                if (f32)
                {
                    lat->weight32.resize(n_cells);
                    std::transform(wts.begin(), wts.end(), lat->weight32.host_write(), [](double b) { return static_cast<float>(b); });
                }
                else
                {
                    lat->weight.resize(n_cells);
                    std::copy(wts.begin(), wts.end(), lat->weight.host_write());
                }
            }
            else if (!map.cell.empty())
            {
                lat->cell.resize(static_cast<int>(map.cell.size()));
                std::copy(map.cell.begin(), map.cell.end(), lat->cell.host_write());
            }
            lat->slots = stride * map.Ly;
            lat->dof_of_slot.resize(lat->slots);
            lat->slot_of_dof.resize(ndof);
            int *dos = lat->dof_of_slot.host_write(), *sod = lat->slot_of_dof.host_write();
            std::fill(dos, dos + lat->slots, -1);
            for (int g = 0; g < ndof; ++g)
            {
                sod[g] = map.node_of[g] % map.Lx + stride * (map.node_of[g] / map.Lx);
                dos[sod[g]] = g;
            }
        }

        // ---- the period's grid
        const int nb = fem.basis().size();
        nt = ratio * detail::coarsened_steps(detail::mesh_grid_steps(omega, fem.mesh().min_h(), nb), scheme.coarsen);
        dt = 2.0 * M_PI / omega / nt;
        filt.resize(nt + 1);
        cs.resize(2 * nt + 1);
        sn.resize(2 * nt + 1);
        detail::fill_time_grid(omega, nt, dt, filt.data(), cs.data(), sn.data());

        // ---- the sweep
        if (lat)
        {
            // the stencil of wave_lattice.hip: no operator, no metric table
        }
        else if (o.stiffness == WaveHoltzOptions::lobatto)
            K.reset(new StiffnessMatrix(fem, fem.basis().quadrature()));
        else
            K.reset(new StiffnessMatrix(fem));

        // ---- invm = 1 / (a^2 m), m the Gauss-Lobatto lumped mass
        const QuadratureRule &gll = fem.basis().quadrature();
        host_device_dvec wts = rule_weights(gll);
        host_device_dvec a2(ndof);
        {
            double *h = a2.host_write();
            for (int g = 0; g < ndof; ++g)
                h[g] = h_a[g] * h_a[g];
        }
        const double *detJ = fem.mesh().element_metrics(gll).measures(MemorySpace::DEVICE);
        detail::check_hip(cuddh_hip_diag_mass_setup(ndof, fem.mesh().n_elem(), nb, a2.device_read(), detJ, wts.device_read(),
                                                    fem.global_indices(MemorySpace::DEVICE), invm.device_write(), stream()),
                          "WaveHoltz lumped mass");

        // ---- Hi = h a on the dofs of the absorbing faces (h the lumped face mass), zero elsewhere
        std::vector<int> all;
        const int *faces = o.h_faces;
        int n_faces = o.n_faces;
        if (n_faces < 0)
        {
            const ivec b = fem.mesh().boundary_edges();
            for (int i = 0; i < b.size(); ++i)
                all.push_back(b[i]);
            faces = all.data();
            n_faces = static_cast<int>(all.size());
        }
        double *d_Hi = Hi.device_write(); // a fresh allocation: zero-filled
        if (n_faces > 0)
        {
            for (int f = 0; f < n_faces; ++f)
                if (faces[f] < 0 || faces[f] >= fem.mesh().n_edges())
                    cuddh_error(("WaveHoltz error: faces: edge " + std::to_string(faces[f]) + " is not an edge of the mesh.").c_str());
            FaceSpace fs(fem, n_faces, faces);
            host_device_dvec af(fs.size()), hf(fs.size());
            {
                double *h = af.host_write();
                const int *proj = fs.global_indices(MemorySpace::HOST);
                for (int i = 0; i < fs.size(); ++i)
                    h[i] = h_a[proj[i]];
            }
            const double *fdetJ = fs.metrics(gll).measures(MemorySpace::DEVICE);
            double *d_hf = hf.device_write(); // zero-filled, which the accumulation needs
            detail::check_hip(cuddh_hip_diag_facemass_setup(fs.size(), n_faces, nb, wts.device_read(), fdetJ, af.device_read(),
                                                            fs.subspace_indices(MemorySpace::DEVICE), d_hf, stream()),
                              "WaveHoltz lumped face mass");
            detail::check_hip(cuddh_hip_reciprocal_f64(fs.size(), d_hf, stream()), "WaveHoltz lumped face mass"); // the set-up leaves 1 / (h a)
            fs.prolong(d_hf, d_Hi);
            detail::check_hip(cuddh_hip_stream_sync(stream()), "WaveHoltz setup"); // fs and its vectors die here
        }
        detail::check_hip(cuddh_hip_stream_sync(stream()), "WaveHoltz setup"); // a2 and wts die here

        const bool rk4 = scheme.scheme == DDHIntegrator::rk4;
        int nvec = ndof;
        if (lat && lat->f32)
        {
            // invm and Hi, set up in double above, into lattice order as floats; the padding slots get zero.  The class's double
            // lattice vectors are not allocated.
            const int n = lat->slots;
            const int *dos = lat->dof_of_slot.device_read();
            lat->invm.resize(n);
            lat->Hi.resize(n);
            detail::check_hip(cuddh_hip_wave32_load(n, dos, invm.device_read(), lat->invm.device_write(), stream()), "WaveHoltz lattice order");
            detail::check_hip(cuddh_hip_wave32_load(n, dos, Hi.device_read(), lat->Hi.device_write(), stream()), "WaveHoltz lattice order");
            detail::check_hip(cuddh_hip_stream_sync(stream()), "WaveHoltz setup"); // the dof-ordered vectors die here
            invm.resize(0);
            Hi.resize(0);
            lat->slot_of_dof.device_read();
            for (HostDeviceArray<float> *x : {&lat->p, &lat->q, &lat->u, &lat->v, &lat->ps, &lat->qs})
                x->resize(n);
            if (rk4)
                for (HostDeviceArray<float> *x : {&lat->ps2f, &lat->aq, &lat->ap})
                    x->resize(n);
            tmp.resize(2 * ndof);
            return;
        }
        if (lat)
        {
            // invm and Hi into lattice order; the padding slots get zero
            nvec = lat->slots;
            const int *dos = lat->dof_of_slot.device_read();
            for (host_device_dvec *x : {&invm, &Hi})
            {
                host_device_dvec t(nvec);
                detail::check_hip(cuddh_hip_wave_lattice_gather_f64(nvec, dos, x->device_read(), t.device_write(), stream()), "WaveHoltz lattice order");
                detail::check_hip(cuddh_hip_stream_sync(stream()), "WaveHoltz setup"); // the dof-ordered vector dies here
                *x = std::move(t);
            }
            lat->slot_of_dof.device_read();
            if (rk4)
                lat->ps2.resize(nvec);
        }
        else
            w.resize(ndof);
        for (host_device_dvec *x : {&p, &q, &u, &v, &ps, &qs})
            x->resize(nvec);
        tmp.resize(2 * ndof);
        if (rk4)
        {
            aq.resize(nvec);
            ap.resize(nvec);
        }
    }

    WaveHoltz::~WaveHoltz() = default;

    std::string WaveHoltz::stiffness_kernel() const
    {
        if (!lat)
            return K->kernel_name();
        const int nb = lat->desc.n_basis;
        return std::string(lat->weighted() ? "wave_weights nb" : lat->pair ? "wave_pair nb" : (lat->cell.size() ? "wave_cells nb" : "wave_lattice nb")) + std::to_string(nb) + (lat->f32 ? " f32" : "") + (nb == 4 || nb == 5 ? "" : " (run-time n_basis)");
    }

    WaveHoltzOptions::Precision WaveHoltz::precision() const { return lat && lat->f32 ? WaveHoltzOptions::f32 : WaveHoltzOptions::f64; }

    WaveHoltzOptions::Launch WaveHoltz::launch() const { return lat && lat->pair ? WaveHoltzOptions::per_pair : WaveHoltzOptions::per_sweep; }

    void WaveHoltz::lattice_period(const double *z_in, const double *f, double *z_out) const
    {
        const int n = lat->slots;
        const bool rk4 = scheme.scheme == DDHIntegrator::rk4;
        const LatticeGrid g = {&lat->desc, n, ndof, nt, rk4, lat->pair, dt, filt.data(), cs.data(), sn.data(), lat->dof_of_slot.device_read(),
                               lat->slot_of_dof.device_read(), stream(), lat->cell.size() ? lat->cell.device_read() : nullptr};
        if (lat->f32)
        {
            Lattice &L = *lat;
            if (f && L.F.size() != n)
            {
                L.F.resize(n);
                L.G.resize(n);
            }
            LatticeVectors<float> x = {{L.p.device_write(), L.q.device_write(), L.u.device_write(), L.v.device_write(), L.ps.device_write(),
                                        L.qs.device_write(), rk4 ? L.ps2f.device_write() : nullptr, rk4 ? L.aq.device_write() : nullptr,
                                        rk4 ? L.ap.device_write() : nullptr, f ? L.F.device_write() : nullptr, f ? L.G.device_write() : nullptr,
                                        L.invm.device_read(), L.Hi.device_read()}};
            if (L.weight32.size())
                x.W = L.weight32.device_read();
            return lattice_march(g, x, z_in, f, z_out);
        }
        if (f && F.size() != n)
        {
            F.resize(n);
            G.resize(n);
        }
        LatticeVectors<double> x = {{p.device_write(), q.device_write(), u.device_write(), v.device_write(), ps.device_write(),
                                     qs.device_write(), rk4 ? lat->ps2.device_write() : nullptr, rk4 ? aq.device_write() : nullptr,
                                     rk4 ? ap.device_write() : nullptr, f ? F.device_write() : nullptr, f ? G.device_write() : nullptr,
                                     invm.device_read(), Hi.device_read()}};
        if (lat->weight.size())
            x.W = lat->weight.device_read();
        lattice_march(g, x, z_in, f, z_out);
    }

    void WaveHoltz::period(const double *z_in, const double *f, double *z_out) const
    {
        if (lat)
            return lattice_period(z_in, f, z_out);
        const int n = ndof;
        void *st = stream();
        double *W = w.device_write(), *P = p.device_write(), *Q = q.device_write(), *U = u.device_write(), *V = v.device_write();
        double *PS = ps.device_write(), *QS = qs.device_write();
        const double *IM = invm.device_read(), *HI = Hi.device_read();
        const double *Ff = nullptr, *Gf = nullptr;
        if (f)
        {
            // copies of the load on 16-byte boundaries (f + ndof is on one only when ndof is even)
            if (F.size() != n)
            {
                F.resize(n);
                G.resize(n);
            }
            double *dF = F.device_write(), *dG = G.device_write();
            copy(n, f, dF);
            copy(n, f + n, dG);
            Ff = dF;
            Gf = dG;
        }
        if (z_in)
            detail::check_hip(cuddh_hip_wave_stage_begin_f64(n, filt[0], z_in, z_in + n, P, Q, U, V, st), "WaveHoltz::period");
        else
            for (double *x : {P, Q, U, V})
                zeros(n, x);

        if (scheme.scheme == DDHIntegrator::rk2)
        {
            for (int it = 1; it <= nt; ++it)
            {
                K->action(P, W);
                detail::check_hip(cuddh_hip_wave_stage_rk2_a_f64(n, 0.5 * dt, cs[2 * it - 2], sn[2 * it - 2], W, P, Q, IM, HI, Ff, Gf, QS, PS, st),
                                  "WaveHoltz::period");
                K->action(PS, W);
                detail::check_hip(cuddh_hip_wave_stage_rk2_b_f64(n, dt, cs[2 * it - 1], sn[2 * it - 1], filt[it], W, QS, IM, HI, Ff, Gf, P, Q, U, V, st),
                                  "WaveHoltz::period");
            }
        }
        else
        {
            double *AQ = aq.device_write(), *AP = ap.device_write();
            for (int it = 1; it <= nt; ++it)
            {
                const int k = 2 * it - 2;
                K->action(P, W);
                detail::check_hip(cuddh_hip_wave_stage_rk4_1_f64(n, 0.5 * dt, cs[k], sn[k], W, P, Q, IM, HI, Ff, Gf, PS, QS, AQ, AP, st), "WaveHoltz::period");
                K->action(PS, W);
                detail::check_hip(cuddh_hip_wave_stage_rk4_2_f64(n, 0.5 * dt, cs[k + 1], sn[k + 1], W, P, Q, IM, HI, Ff, Gf, PS, QS, AQ, AP, st),
                                  "WaveHoltz::period");
                K->action(PS, W);
                detail::check_hip(cuddh_hip_wave_stage_rk4_3_f64(n, dt, cs[k + 1], sn[k + 1], W, P, Q, IM, HI, Ff, Gf, PS, QS, AQ, AP, st), "WaveHoltz::period");
                K->action(PS, W);
                detail::check_hip(cuddh_hip_wave_stage_rk4_4_f64(n, dt / 6.0, cs[k + 2], sn[k + 2], filt[it], W, QS, AQ, AP, IM, HI, Ff, Gf, P, Q, U, V, st),
                                  "WaveHoltz::period");
            }
        }
        copy(n, U, z_out);
        copy(n, V, z_out + n);
    }

    void WaveHoltz::solution(const double *z, double *out) const
    {
        if (out != z)
            copy(2 * ndof, z, out);
        scal(ndof, 1.0 / omega, out + ndof);
    }

    void WaveHoltz::action(const double *x, double *y) const
    {
        period(x, nullptr, y);
        axpby(2 * ndof, 1.0, x, -1.0, y);
    }

    void WaveHoltz::action(double c, const double *x, double *y) const
    {
        double *t = tmp.device_write();
        period(x, nullptr, t);
        axpby(2 * ndof, c, x, 1.0, y);
        axpby(2 * ndof, -c, t, 1.0, y);
    }
} // namespace cuddh
