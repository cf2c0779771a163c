// DDH set-up (host) and the three entry points rhs / action / postprocess.
// Set-up rules restated from reference source/DDH.cpp:323-609; the local solves
// themselves are the HIP kernels behind cuddh_hip_ddh_apply_*.
#include "cuddh/ddh.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "cuddh/parallel.hpp"
#include "cuddh/time_grid.hpp"
#include "cuddh_hip.h"

namespace cuddh
{
    namespace detail
    {
        namespace
        {
            template <typename Real>
            void geom_setup(int n_domains, int mx_elems, int nb, const int *n_elems, const int *elems, const double *w,
                            const double *points, const double *corners, Real *G)
            {
                int err;
                if constexpr (std::is_same_v<Real, float>)
                    err = cuddh_hip_ddh_geom_from_corners_f32(n_domains, mx_elems, nb, n_elems, elems, w, points, corners, G, stream());
                else
                    err = cuddh_hip_ddh_geom_from_corners_f64(n_domains, mx_elems, nb, n_elems, elems, w, points, corners, G, stream());
                check_hip(err, "DDH geometric factors");
            }

            /// what can be refused about a time-step policy without the subdomains' dofs: all of it
            void check_time_step(const DDHTimeStep &ts, const double *h_a, int g_ndof, int n_domains)
            {
                if (ts.policy == DDHTimeStep::mesh)
                    return;
                if (ts.policy == DDHTimeStep::ratios)
                {
                    if (!ts.h_ratios || ts.n_ratios != n_domains)
                        cuddh_error(("DDH error: time step: " + std::to_string(ts.h_ratios ? ts.n_ratios : 0) + " ratios for " +
                                     std::to_string(n_domains) + " subdomains.").c_str());
                    for (int s = 0; s < n_domains; ++s)
                        if (ts.h_ratios[s] < 1 || ts.h_ratios[s] > DDHTimeStep::max_ratio)
                            cuddh_error(("DDH error: time step: ratio " + std::to_string(ts.h_ratios[s]) + " of subdomain " + std::to_string(s) +
                                         " is outside [1, " + std::to_string(DDHTimeStep::max_ratio) + "].").c_str());
                    return;
                }
                if (ts.policy != DDHTimeStep::coefficient)
                    cuddh_error("DDH error: time step: unknown policy.");
                // every dof lies in some subdomain: the smallest a of all is some subdomain's smallest
                double a_min = INFINITY;
                for (int g = 0; g < g_ndof; ++g)
                {
                    if (!std::isfinite(h_a[g]) || !(h_a[g] > 0.0))
                        cuddh_error(("DDH error: time step: a = " + std::to_string(h_a[g]) + " at dof " + std::to_string(g) +
                                     "; the time step from the coefficient needs a finite and positive.").c_str());
                    a_min = std::min(a_min, h_a[g]);
                }
                if (g_ndof > 0 && std::ceil((1.0 / a_min) * (1.0 - 1e-9)) > DDHTimeStep::max_ratio)
                    cuddh_error(("DDH error: time step: min a = " + std::to_string(a_min) + " asks for more than " +
                                 std::to_string(DDHTimeStep::max_ratio) + " times the mesh grid's steps.").c_str());
            }
        } // namespace

        template <typename Real>
        struct DDHCore<Real>::More
        {
            const Basis *fem_basis;
            int nt_mesh = 0;                                     // steps of the mesh grid; subdomain s marches ratios[s] * nt_mesh
            std::vector<int> ratios, grid_ratio;                 // per subdomain; distinct and ascending (empty: one grid)
            std::vector<long long> grid_filter_off, grid_cs_off; // grid g's tables within the concatenated ones below
            host_device_ivec grid_of;
            HostDeviceArray<Real> grid_filter, grid_cs, grid_sn;

            DDHIntegrator integrator;                            // rk4: nt_mesh is the coarsened count, ceil(mesh grid's / coarsen)

            explicit More(const Basis *basis) : fem_basis(basis) {}
        };

        template <typename Real>
        int DDHCore<Real>::mesh_steps() const { return more->nt_mesh; }
        template <typename Real>
        DDHIntegrator DDHCore<Real>::integrator() const { return more->integrator; }
        template <typename Real>
        const std::vector<int> &DDHCore<Real>::time_ratios() const { return more->ratios; }
        template <typename Real>
        const std::vector<int> &DDHCore<Real>::time_grid_ratios() const { return more->grid_ratio; }

        template <typename Real>
        DDHCore<Real>::DDHCore(double omega_, const double *h_a, const H1Space &fem, int nx, int ny, int kernel)
            : g_ndof(fem.size()), g_elem(fem.mesh().n_elem()), n_basis(fem.basis().size()), omega(omega_), fem_mesh(&fem.mesh()),
              more(new More(&fem.basis()))
        {
            const int nb = n_basis;
            if (nb < 2 || nb > 16)
                cuddh_error("DDH error: n_basis must be in [2, 16].");

            // ---- blocks of nel1d x nel1d elements (16 / nb per side: <= 256 nodes per subdomain)
            nel1d = std::max(1, 16 / nb);
            if (nx % nel1d != 0 || ny % nel1d != 0)
                cuddh_error("DDH error: nx and ny must be multiples of 16 / n_basis.");
            setup_blocks(h_a, fem, nx, ny);
            requested_kernel = kernel;
        }

        template <typename Real>
        DDHCore<Real>::DDHCore(double omega_, const double *h_a, const H1Space &fem, int nx, int ny, int kernel, int block)
            : g_ndof(fem.size()), g_elem(fem.mesh().n_elem()), n_basis(fem.basis().size()), omega(omega_), fem_mesh(&fem.mesh()),
              more(new More(&fem.basis()))
        {
            // everything is checked here, on the host, before anything is allocated or launched
            set_block(nx, ny, block);
            setup_blocks(h_a, fem, nx, ny);
            requested_kernel = kernel;
        }

        template <typename Real>
        void DDHCore<Real>::set_block(int nx, int ny, int block)
        {
            const int nb = n_basis;
            if (nb < 2 || nb > 16)
                cuddh_error("DDH error: n_basis must be in [2, 16].");
            if (block < 0)
                cuddh_error(("DDH error: block = " + std::to_string(block) + "; the elements per subdomain side must be at least 1 (0: 16 / n_basis).").c_str());
            nel1d = block == 0 ? std::max(1, 16 / nb) : block;
            if (static_cast<long long>(nb) * nb * nel1d * nel1d > 1024)
                cuddh_error(("DDH error: block = " + std::to_string(nel1d) + " at n_basis " + std::to_string(nb) + " gives " +
                             std::to_string(static_cast<long long>(nb) * nb * nel1d * nel1d) +
                             " element nodes per subdomain (n_basis^2 * block^2); at most 1024 fit one local solve.")
                                .c_str());
            if (nx % nel1d != 0 || ny % nel1d != 0)
                cuddh_error(("DDH error: nx = " + std::to_string(nx) + " and ny = " + std::to_string(ny) + " must be multiples of block = " +
                             std::to_string(nel1d) + ".")
                                .c_str());
        }

        template <typename Real>
        DDHCore<Real>::DDHCore(double omega_, const double *h_a, const H1Space &fem, int nx, int ny, int kernel, int block,
                               const DDHTimeStep &time_step)
            : g_ndof(fem.size()), g_elem(fem.mesh().n_elem()), n_basis(fem.basis().size()), omega(omega_), fem_mesh(&fem.mesh()),
              more(new More(&fem.basis()))
        {
            // the checks of the constructor above, then the policy's: all on the host, before anything is allocated or launched
            set_block(nx, ny, block);
            if (nx * ny != g_elem)
                cuddh_error("DDH error: nx * ny does not match the mesh.");
            check_time_step(time_step, h_a, g_ndof, (nx / nel1d) * (ny / nel1d));
            setup_blocks(h_a, fem, nx, ny, time_step);
            requested_kernel = kernel;
        }

        template <typename Real>
        DDHCore<Real>::DDHCore(double omega_, const double *h_a, const H1Space &fem, int nx, int ny, int kernel, int block,
                               const DDHTimeStep &time_step, const DDHIntegrator &integrator)
            : g_ndof(fem.size()), g_elem(fem.mesh().n_elem()), n_basis(fem.basis().size()), omega(omega_), fem_mesh(&fem.mesh()),
              more(new More(&fem.basis()))
        {
            // the integrator's checks first, then those of the constructor above: all on the host
            set_integrator(integrator);
            set_block(nx, ny, block);
            if (nx * ny != g_elem)
                cuddh_error("DDH error: nx * ny does not match the mesh.");
            check_time_step(time_step, h_a, g_ndof, (nx / nel1d) * (ny / nel1d));
            setup_blocks(h_a, fem, nx, ny, time_step);
            requested_kernel = kernel;
        }

        template <typename Real>
        void DDHCore<Real>::set_integrator(const DDHIntegrator &integrator)
        {
            if (integrator.scheme != DDHIntegrator::rk2 && integrator.scheme != DDHIntegrator::rk4)
                cuddh_error("DDH error: integrator: the scheme must be rk2 or rk4.");
            if (integrator.coarsen < 1 || integrator.coarsen > DDHIntegrator::max_coarsen)
                cuddh_error(("DDH error: integrator: coarsen = " + std::to_string(integrator.coarsen) + " is outside [1, " +
                             std::to_string(DDHIntegrator::max_coarsen) + "].").c_str());
            if (integrator.scheme == DDHIntegrator::rk2 && integrator.coarsen != 1)
                cuddh_error("DDH error: integrator: rk2 marches on the mesh grid (coarsen = 1) only; a coarser grid needs rk4.");
            more->integrator = integrator;
        }

        template <typename Real>
        void DDHCore<Real>::setup_blocks(const double *h_a, const H1Space &fem, int nx, int ny, const DDHTimeStep &time_step)
        {
            if (nx * ny != g_elem)
                cuddh_error("DDH error: nx * ny does not match the mesh.");

            const int ndx = nx / nel1d, ndy = ny / nel1d;
            n_domains = ndx * ndy;
            std::vector<int> labels(static_cast<std::size_t>(nx) * ny);
            parallel_for(static_cast<std::size_t>(ny), [&](std::size_t j0, std::size_t j1, int)
            {
                for (int j = static_cast<int>(j0); j < static_cast<int>(j1); ++j)
                    for (int i = 0; i < nx; ++i)
                        labels[i + static_cast<std::size_t>(nx) * j] = (i / nel1d) + ndx * (j / nel1d);
            }, 8);
            setup(h_a, fem, labels.data(), time_step);
        }

        template <typename Real>
        DDHCore<Real>::DDHCore(from_labels_t tag, double omega_, const double *h_a, const H1Space &fem, int n_domains_, const int *labels,
                               int kernel)
            : DDHCore(tag, omega_, h_a, fem, n_domains_, labels, kernel, DDHTimeStep::from_mesh(), DDHIntegrator{})
        {
        }

        template <typename Real>
        DDHCore<Real>::DDHCore(from_labels_t, double omega_, const double *h_a, const H1Space &fem, int n_domains_, const int *labels,
                               int kernel, const DDHTimeStep &time_step, const DDHIntegrator &integrator)
            : g_ndof(fem.size()), g_elem(fem.mesh().n_elem()), n_basis(fem.basis().size()), n_domains(n_domains_), nel1d(0),
              omega(omega_), fem_mesh(&fem.mesh()), more(new More(&fem.basis())), requested_kernel(kernel), general(true)
        {
            // everything is checked here, on the host, before anything is allocated or launched: the integrator, the labels,
            // then the time-step policy
            set_integrator(integrator);
            const int nb = n_basis;
            if (nb < 2 || nb > 10)
                cuddh_error("DDH error: subdomains from labels need n_basis in [2, 10].");
            if (n_domains < 1)
                cuddh_error("DDH error: n_domains must be at least 1.");
            if (!labels)
                cuddh_error("DDH error: no element labels.");
            std::vector<int> count(n_domains, 0);
            for (int el = 0; el < g_elem; ++el)
            {
                const int s = labels[el];
                if (s < 0 || s >= n_domains)
                    cuddh_error(("DDH error: element " + std::to_string(el) + " has label " + std::to_string(s) + ", outside [0, " +
                                 std::to_string(n_domains) + ").").c_str());
                ++count[s];
            }
            int mx_elems = 0;
            for (int s = 0; s < n_domains; ++s)
            {
                if (count[s] == 0)
                    cuddh_error(("DDH error: subdomain " + std::to_string(s) + " has no elements.").c_str());
                if (nb * nb * count[s] > 256)
                    cuddh_error(("DDH error: subdomain " + std::to_string(s) + " has " + std::to_string(nb * nb * count[s]) +
                                 " element nodes (n_basis^2 * " + std::to_string(count[s]) + " elements); at most 256 fit one local solve.")
                                    .c_str());
                mx_elems = std::max(mx_elems, count[s]);
            }
            if (kernel != 0 && kernel != 9 && kernel != 10)
                cuddh_error("DDH error: subdomains from labels run kernel 9 or 10 (0 = auto); kernels 1-8 need the block grid.");
            if (kernel == 9 && (nb != 4 || mx_elems > 16))
                cuddh_error("DDH error: kernel 9 needs n_basis 4 and at most 16 elements per subdomain.");
            check_time_step(time_step, h_a, g_ndof, n_domains);
            setup(h_a, fem, labels, time_step);
        }

        template <typename Real>
        void DDHCore<Real>::setup_time_grids(const double *h_a, const H1Space &fem, const DDHTimeStep &time_step)
        {
            const int nb = n_basis;
            int &nt_mesh = more->nt_mesh;
            std::vector<int> &ratios = more->ratios, &grid_ratio = more->grid_ratio;
            std::vector<long long> &grid_filter_off = more->grid_filter_off, &grid_cs_off = more->grid_cs_off;
            host_device_ivec &_grid_of = more->grid_of;
            HostDeviceArray<Real> &_grid_filter = more->grid_filter, &_grid_cs = more->grid_cs, &_grid_sn = more->grid_sn;
            // ---- the mesh grid: dt = 0.1 h / nb^2 shrunk so that nt dt is one period
            const double T = 2.0 * M_PI / omega;
            const double h = fem.mesh().min_h();
            nt = nt_mesh = mesh_grid_steps(omega, h, nb);
            // RK4 on a coarser grid: ceil(nt_mesh / coarsen) steps are the base grid, and what the ratios below multiply
            if (const int c = more->integrator.coarsen; c > 1)
                nt = nt_mesh = coarsened_steps(nt_mesh, c);

            // ---- steps of subdomain s = ratios[s] * nt_mesh
            ratios.assign(n_domains, 1);
            if (time_step.policy == DDHTimeStep::ratios)
                ratios.assign(time_step.h_ratios, time_step.h_ratios + n_domains);
            else if (time_step.policy == DDHTimeStep::coefficient)
            {
                // the wave speed is 1 / a: the smallest a among the subdomain's dofs, those it shares with its neighbours
                // included, sets its step.  (1 - 1e-9) keeps 1 / a that is an integer up to rounding (a = 0.2) on that integer
                auto sizes = efem->sizes(MemorySpace::HOST);
                auto gI = reshape(_gI.host_read(), mx_dof, n_domains);
                for (int s = 0; s < n_domains; ++s)
                {
                    double a_min = INFINITY;
                    for (int i = 0; i < sizes(s); ++i)
                        a_min = std::min(a_min, h_a[gI(i, s)]);
                    ratios[s] = ratio_from_coefficient(a_min);
                }
            }
            std::vector<int> distinct(ratios);
            std::sort(distinct.begin(), distinct.end());
            distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
            // one ratio for all under `coefficient`: a plain plan on that grid.  Ratios given one by one are honoured as given.
            const bool per_subdomain = time_step.policy == DDHTimeStep::ratios || (time_step.policy == DDHTimeStep::coefficient && distinct.size() > 1);
            if (time_step.policy == DDHTimeStep::coefficient && !per_subdomain)
                nt = distinct[0] * nt_mesh;
            dt = T / nt;

            _wh_filter.resize(nt + 1);
            _cs.resize(2 * nt + 1);
            _sn.resize(2 * nt + 1);
            fill_time_grid(omega, nt, dt, _wh_filter.host_write(), _cs.host_write(), _sn.host_write());
            if (!per_subdomain)
                return;

            grid_ratio = distinct;
            long long n_filter = 0, n_cs = 0;
            for (const int r : grid_ratio)
            {
                grid_filter_off.push_back(n_filter);
                grid_cs_off.push_back(n_cs);
                n_filter += static_cast<long long>(r) * nt_mesh + 1;
                n_cs += 2LL * r * nt_mesh + 1;
            }
            if (n_cs > 2147483647LL)
                cuddh_error("DDH error: time step: the time grids' tables need more than 2^31 entries.");
            _grid_filter.resize(static_cast<int>(n_filter));
            _grid_cs.resize(static_cast<int>(n_cs));
            _grid_sn.resize(static_cast<int>(n_cs));
            Real *gf = _grid_filter.host_write(), *gc = _grid_cs.host_write(), *gs = _grid_sn.host_write();
            for (std::size_t g = 0; g < grid_ratio.size(); ++g)
            {
                const int nt_g = grid_ratio[g] * nt_mesh;
                fill_time_grid(omega, nt_g, T / nt_g, gf + grid_filter_off[g], gc + grid_cs_off[g], gs + grid_cs_off[g]);
            }
            _grid_of.resize(n_domains);
            int *grid_of = _grid_of.host_write();
            for (int s = 0; s < n_domains; ++s)
                grid_of[s] = static_cast<int>(std::lower_bound(grid_ratio.begin(), grid_ratio.end(), ratios[s]) - grid_ratio.begin());
        }

        template <typename Real>
        long long DDHCore<Real>::time_grid_table(int ratio, int which, const Real *&table) const
        {
            const int nt_mesh = more->nt_mesh;
            const std::vector<int> &grid_ratio = more->grid_ratio;
            const std::vector<long long> &grid_filter_off = more->grid_filter_off, &grid_cs_off = more->grid_cs_off;
            const HostDeviceArray<Real> &_grid_filter = more->grid_filter, &_grid_cs = more->grid_cs, &_grid_sn = more->grid_sn;
            if (which < 0 || which > 2 || ratio < 1)
                return 0;
            const long long n = (which == 0 ? 1LL : 2LL) * ratio * nt_mesh + 1;
            if (grid_ratio.empty())
            {
                if (static_cast<long long>(ratio) * nt_mesh != nt)
                    return 0;
                table = which == 0 ? _wh_filter.host_read() : which == 1 ? _cs.host_read() : _sn.host_read();
                return n;
            }
            const auto it = std::lower_bound(grid_ratio.begin(), grid_ratio.end(), ratio);
            if (it == grid_ratio.end() || *it != ratio)
                return 0;
            const std::size_t g = it - grid_ratio.begin();
            table = which == 0 ? _grid_filter.host_read() + grid_filter_off[g]
                               : (which == 1 ? _grid_cs.host_read() : _grid_sn.host_read()) + grid_cs_off[g];
            return n;
        }

        template <typename Real>
        void DDHCore<Real>::setup(const double *h_a, const H1Space &fem, const int *labels, const DDHTimeStep &time_step)
        {
            const int nb = n_basis;
            PhaseTimer timer;
            efem.reset(new EnsembleSpace(fem, n_domains, labels));
            timer.lap("EnsembleSpace");

            // ---- extents
            auto sizes = efem->sizes(MemorySpace::HOST);
            auto fsizes = efem->fsizes(MemorySpace::HOST);
            auto s_nel = efem->n_elems(MemorySpace::HOST);
            mx_dof = mx_fdof = mx_elem_per_dom = 0;
            for (int s = 0; s < n_domains; ++s)
            {
                mx_dof = std::max(mx_dof, sizes(s));
                mx_fdof = std::max(mx_fdof, fsizes(s));
                mx_elem_per_dom = std::max(mx_elem_per_dom, s_nel(s));
            }

            // ---- trace slots.  lambda = (l0, l1, m0, m1): pair k of cmap owns slot k on its first
            // subdomain's side and slot n_shared + k on the second's; each side reads its own slot and
            // writes the other's.  Later pairs overwrite earlier ones at cross points (reference quirk:
            // source/DDH.cpp:436-439), which leaves a few slots unused.
            auto cmap = efem->connectivity_map(MemorySpace::HOST);
            const int n_shared = cmap.shape(1);
            n_lambda = 2 * n_shared;

            _Bf.resize(2 * mx_fdof * n_domains);
            auto B = reshape(_Bf.host_write(), mx_fdof, 2, n_domains);
            std::fill(B.begin(), B.end(), -1);
            for (int k = 0; k < n_shared; ++k)
            {
                const int S0 = cmap(0, k), S1 = cmap(1, k), j0 = cmap(2, k), j1 = cmap(3, k);
                B(j0, 0, S0) = k;
                B(j0, 1, S0) = n_shared + k;
                B(j1, 0, S1) = n_shared + k;
                B(j1, 1, S1) = k;
            }

            timer.lap("trace slots");
            // ---- renumber each subdomain so that its face dofs come first (in face-space order)
            auto faceproj = efem->face_proj(MemorySpace::HOST);
            auto g_inds = efem->global_indices(MemorySpace::HOST);
            auto s_inds = efem->subspace_indices(MemorySpace::HOST);
            auto s_elems = efem->elements(MemorySpace::HOST);

            _gI.resize(mx_dof * n_domains);
            auto gI = reshape(_gI.host_write(), mx_dof, n_domains);
            _sI.resize(nb * nb * mx_elem_per_dom * n_domains);
            auto sI = reshape(_sI.host_write(), nb, nb, mx_elem_per_dom, n_domains);
            std::fill(sI.begin(), sI.end(), -1); // element nodes past a smaller subdomain's elements

            parallel_for(static_cast<std::size_t>(n_domains), [&](std::size_t s0, std::size_t s1, int)
            {
                std::vector<int> new_of_old(mx_dof);
                for (int s = static_cast<int>(s0); s < static_cast<int>(s1); ++s)
                {
                    const int nd = sizes(s), nf = fsizes(s);
                    std::fill(new_of_old.begin(), new_of_old.end(), -1);
                    int next = 0;
                    for (; next < nf; ++next)
                    {
                        const int old = faceproj(next, s);
                        new_of_old[old] = next;
                        gI(next, s) = g_inds(old, s);
                    }
                    for (int old = 0; old < nd; ++old)
                        if (new_of_old[old] < 0)
                        {
                            new_of_old[old] = next;
                            gI(next, s) = g_inds(old, s);
                            ++next;
                        }
                    for (int el = 0; el < s_nel(s); ++el)
                        for (int l = 0; l < nb; ++l)
                            for (int k = 0; k < nb; ++k)
                                sI(k, l, el, s) = new_of_old[s_inds(k, l, el, s)];
                }
            }, 16);

            timer.lap("face-first renumbering");
            setup_time_grids(h_a, fem, time_step);
            timer.lap("time grid tables");
            // ---- local operators
            const Basis &basis = fem.basis();
            const QuadratureRule &q = basis.quadrature();

            _D.resize(nb * nb);
            {
                dmat Dd(nb, nb);
                basis.deriv(nb, q.x(), Dd);
                Real *hD = _D.host_write();
                for (int i = 0; i < nb * nb; ++i)
                    hD[i] = static_cast<Real>(Dd[i]);
            }

            // det J at the GLL points, evaluated where it is used (the reference reads the tabulated array,
            // source/DDH.cpp:551-552; tabulating 16 n_elem doubles on the host costs more than the two loops that read them)
            const Mesh2D &the_mesh = fem.mesh();
            auto detJ = [&](int i, int j, int el)
            {
                const double xi[2] = {q.x(i), q.x(j)};
                return the_mesh.element(el)->measure(xi);
            };
            auto fem_gi = fem.global_indices(MemorySpace::HOST);

            timer.lap("element metrics");
            // global lumped mass and its inverse.  The reference adds the element contributions of a dof in element order
            // (source/DDH.cpp:559-566); to keep that order (and with it every bit of the sum) with several threads, a dof
            // touched by ONE range of elements is summed by that range, the few touched by several ranges afterwards, serially.
            std::vector<double> inv_mass(g_ndof, 0.0);
            {
                const int nn = nb * nb;
                std::vector<std::atomic<int>> toucher(g_ndof); // -1 none, c one range, -2 several
                parallel_for(static_cast<std::size_t>(g_ndof), [&](std::size_t g0, std::size_t g1, int)
                {
                    for (std::size_t g = g0; g < g1; ++g)
                        toucher[g].store(-1, std::memory_order_relaxed);
                });
                parallel_for(static_cast<std::size_t>(g_elem), [&](std::size_t e0, std::size_t e1, int c)
                {
                    for (std::size_t v = e0 * nn; v < e1 * nn; ++v)
                    {
                        std::atomic<int> &t = toucher[fem_gi[v]];
                        int cur = t.load(std::memory_order_relaxed);
                        while (cur != c && cur != -2 && !t.compare_exchange_weak(cur, cur == -1 ? c : -2, std::memory_order_relaxed))
                        {
                        }
                    }
                }, 64);
                const int C = chunk_count(static_cast<std::size_t>(g_elem), 64);
                std::vector<std::vector<int>> seam(C); // elements with a dof that several ranges touch, per range, in order
                parallel_for(static_cast<std::size_t>(g_elem), [&](std::size_t e0, std::size_t e1, int c)
                {
                    for (int el = static_cast<int>(e0); el < static_cast<int>(e1); ++el)
                    {
                        bool on_seam = false;
                        for (int j = 0; j < nb; ++j)
                            for (int i = 0; i < nb; ++i)
                            {
                                const int g = fem_gi(i, j, el);
                                if (toucher[g].load(std::memory_order_relaxed) == -2)
                                    on_seam = true;
                                else
                                    inv_mass[g] += q.w(i) * q.w(j) * detJ(i, j, el);
                            }
                        if (on_seam)
                            seam[c].push_back(el);
                    }
                }, 64);
                for (int c = 0; c < C; ++c)
                    for (const int el : seam[c])
                        for (int j = 0; j < nb; ++j)
                            for (int i = 0; i < nb; ++i)
                            {
                                const int g = fem_gi(i, j, el);
                                if (toucher[g].load(std::memory_order_relaxed) == -2)
                                    inv_mass[g] += q.w(i) * q.w(j) * detJ(i, j, el);
                            }
                parallel_for(static_cast<std::size_t>(g_ndof), [&](std::size_t g0, std::size_t g1, int)
                {
                    for (std::size_t g = g0; g < g1; ++g)
                        inv_mass[g] = 1.0 / inv_mass[g];
                });
            }

            _m.resize(mx_dof * n_domains);
            _H.resize(mx_fdof * n_domains);
            _a.resize(mx_dof * n_domains);
            _gmi.resize(mx_dof * n_domains);
            auto m = reshape(_m.host_write(), mx_dof, n_domains);
            auto H = reshape(_H.host_write(), mx_fdof, n_domains);
            auto A = reshape(_a.host_write(), mx_dof, n_domains);
            auto gmi = reshape(_gmi.host_write(), mx_dof, n_domains);

            auto faces = efem->faces(MemorySpace::HOST);
            auto n_faces = efem->n_faces(MemorySpace::HOST);
            auto f_inds = efem->face_indices(MemorySpace::HOST);

            parallel_for(static_cast<std::size_t>(n_domains), [&](std::size_t s0, std::size_t s1, int)
            {
                for (int s = static_cast<int>(s0); s < static_cast<int>(s1); ++s)
                {
                    // the storage type accumulates, as in the reference (float += double)
                    for (int el = 0; el < s_nel(s); ++el)
                    {
                        const int g_el = s_elems(el, s);
                        for (int j = 0; j < nb; ++j)
                            for (int i = 0; i < nb; ++i)
                            {
                                Real &acc = m(sI(i, j, el, s), s);
                                acc = static_cast<Real>(acc + q.w(i) * q.w(j) * detJ(i, j, g_el));
                            }
                    }
                    for (int i = 0; i < sizes(s); ++i)
                    {
                        A(i, s) = static_cast<Real>(h_a[gI(i, s)]);
                        gmi(i, s) = static_cast<Real>(inv_mass[gI(i, s)]);
                    }
                    for (int f = 0; f < n_faces(s); ++f)
                    {
                        const Edge *edge = fem.mesh().edge(faces(f, s));
                        for (int i = 0; i < nb; ++i)
                        {
                            Real &acc = H(f_inds(i, f, s), s);
                            acc = static_cast<Real>(acc + edge->measure(q.x(i)) * q.w(i));
                        }
                    }
                }
            }, 16);

            timer.lap("lumped masses, H, a");
        }

        template <typename Real>
        DDHCore<Real>::~DDHCore()
        {
            if (plan)
                cuddh_hip_ddh_plan_destroy(plan);
        }

        template <typename Real>
        void DDHCore<Real>::ensure_plan() const
        {
            if (plan)
                return;
            PhaseTimer timer;
            const int nb = n_basis;
            const QuadratureRule &q = more->fem_basis->quadrature();

            // geometric factors G (3, nb*nb*mx_elems, n_domains) from the Jacobians at the GLL points
            host_device_dvec w(nb);
            double *hw = w.host_write();
            for (int i = 0; i < nb; ++i)
                hw[i] = q.w(i);
            // (the reference reads the tabulated Jacobians, source/DDH.cpp:530-537; here the kernel evaluates the bilinear map from
            // the corners: the 0.5 GB table at 1024^2 is neither built nor kept)
            const auto &metrics = fem_mesh->element_metrics(q);
            const double *d_corners = metrics.corner_coordinates_device();
            check_hip(cuddh_hip_stream_sync(stream()), "DDH element corners");
            timer.lap("plan: element corners to the device");
            _g_tensor.resize(3 * nb * nb * mx_elem_per_dom * n_domains);
            geom_setup<Real>(n_domains, mx_elem_per_dom, nb, efem->n_elems(MemorySpace::DEVICE), efem->elements(MemorySpace::DEVICE),
                             w.device_read(), metrics.rule_nodes_device(), d_corners, _g_tensor.device_write());
            check_hip(cuddh_hip_stream_sync(stream()), "DDH geometric factors");
            timer.lap("plan: geometric factors");

            cuddh_ddh_desc d;
            d.g_ndof = g_ndof;
            d.n_domains = n_domains;
            d.n_lambda = n_lambda;
            d.nb = nb;
            d.nel1d = nel1d;
            d.mx_dof = mx_dof;
            d.mx_fdof = mx_fdof;
            d.nt = nt;
            d.omega = omega;
            d.dt = dt;
            d.s_dof = efem->sizes(MemorySpace::DEVICE);
            d.s_fdof = efem->fsizes(MemorySpace::DEVICE);
            d.B = _Bf.device_read();
            d.gI = _gI.device_read();
            d.sI = _sI.device_read();
            d.D = _D.device_read();
            d.G = _g_tensor.device_read();
            d.m = _m.device_read();
            d.gmi = _gmi.device_read();
            d.a = _a.device_read();
            d.H = _H.device_read();
            d.wh_filter = _wh_filter.device_read();
            d.cs = _cs.device_read();
            d.sn = _sn.device_read();
            const int nt_mesh = more->nt_mesh;
            const std::vector<int> &grid_ratio = more->grid_ratio;
            const host_device_ivec &_grid_of = more->grid_of;
            const HostDeviceArray<Real> &_grid_filter = more->grid_filter, &_grid_cs = more->grid_cs, &_grid_sn = more->grid_sn;
            const bool per_subdomain = !grid_ratio.empty();
            const Real *d_filter = nullptr, *d_cs = nullptr, *d_sn = nullptr;
            const int *d_grid_of = nullptr;
            if (per_subdomain)
            {
                d_filter = _grid_filter.device_read();
                d_cs = _grid_cs.device_read();
                d_sn = _grid_sn.device_read();
                d_grid_of = _grid_of.device_read();
            }
            check_hip(cuddh_hip_stream_sync(stream()), "DDH table upload");
            timer.lap("plan: table uploads");
            const int is_f64 = std::is_same_v<Real, double> ? 1 : 0;
            if (general)
                check_hip(cuddh_hip_ddh_plan_create_general(&plan, &d, mx_elem_per_dom, is_f64, requested_kernel), "DDH plan");
            else
                check_hip(cuddh_hip_ddh_plan_create(&plan, &d, is_f64, requested_kernel), "DDH plan");
            if (more->integrator.scheme == DDHIntegrator::rk4)
            {
                const int err = cuddh_hip_ddh_plan_set_integrator(plan, 1);
                if (err) // never a plan that would step with RK2 instead
                {
                    cuddh_hip_ddh_plan_destroy(plan);
                    plan = nullptr;
                }
                check_hip(err, "DDH integrator (the requested kernel has no RK4 form?)");
            }
            if (per_subdomain)
            {
                std::vector<int> h_nt;
                std::vector<double> h_dt;
                for (const int r : grid_ratio)
                {
                    h_nt.push_back(r * nt_mesh);
                    h_dt.push_back(2.0 * M_PI / omega / h_nt.back());
                }
                const int err = cuddh_hip_ddh_plan_set_time_grids(plan, static_cast<int>(h_nt.size()), h_nt.data(), h_dt.data(), d_filter, d_cs,
                                                                  d_sn, d_grid_of);
                if (err) // never a plan that would march every subdomain on the mesh grid instead
                {
                    cuddh_hip_ddh_plan_destroy(plan);
                    plan = nullptr;
                }
                check_hip(err, "DDH time grids (the requested kernel holds several subdomains per wavefront?)");
            }
            timer.lap("plan: structure check + kernel tables");
        }

        template <typename Real>
        int DDHCore<Real>::kernel_kind() const
        {
            ensure_plan();
            return cuddh_hip_ddh_plan_kernel(plan);
        }

        template <typename Real>
        void DDHCore<Real>::set_waveholtz_iterations(int n) const
        {
            ensure_plan();
            check_hip(cuddh_hip_ddh_plan_set_wh_iters(plan, n), "DDH WaveHoltz iterations");
        }

        template <typename Real>
        void DDHCore<Real>::set_sweep_form(int form) const
        {
            ensure_plan();
            check_hip(cuddh_hip_ddh_plan_set_sweep_form(plan, form), "DDH sweep form");
        }

        template <typename Real>
        int DDHCore<Real>::sweep_form() const
        {
            ensure_plan();
            return cuddh_hip_ddh_plan_sweep_form(plan);
        }

        template <typename Real>
        void DDHCore<Real>::set_chain_order(int order) const
        {
            ensure_plan();
            check_hip(cuddh_hip_ddh_plan_set_chain_order(plan, order), "DDH chain order");
        }

        template <typename Real>
        int DDHCore<Real>::chain_order() const
        {
            ensure_plan();
            return cuddh_hip_ddh_plan_chain_order(plan);
        }

        template <typename Real>
        void DDHCore<Real>::set_forcing(int forcing) const
        {
            ensure_plan();
            check_hip(cuddh_hip_ddh_plan_set_forcing(plan, forcing), "DDH forcing");
        }

        template <typename Real>
        int DDHCore<Real>::forcing() const
        {
            ensure_plan();
            return cuddh_hip_ddh_plan_forcing(plan);
        }

        template <typename Real>
        void DDHCore<Real>::set_march(int march) const
        {
            ensure_plan();
            check_hip(cuddh_hip_ddh_plan_set_march(plan, march), "DDH march");
        }

        template <typename Real>
        int DDHCore<Real>::march() const
        {
            ensure_plan();
            return cuddh_hip_ddh_plan_march(plan);
        }

        template <typename Real>
        void DDHCore<Real>::set_head(int head) const
        {
            ensure_plan();
            check_hip(cuddh_hip_ddh_plan_set_head(plan, head), "DDH head");
        }

        template <typename Real>
        int DDHCore<Real>::head() const
        {
            ensure_plan();
            return cuddh_hip_ddh_plan_head(plan);
        }

        template <typename Real>
        void DDHCore<Real>::set_assembly(int assembly) const
        {
            ensure_plan();
            check_hip(cuddh_hip_ddh_plan_set_assembly(plan, assembly), "DDH assembly");
        }

        template <typename Real>
        int DDHCore<Real>::assembly() const
        {
            ensure_plan();
            return cuddh_hip_ddh_plan_assembly(plan);
        }

        template <typename Real>
        void DDHCore<Real>::set_last_copy_publishes(bool last) const
        {
            ensure_plan();
            check_hip(cuddh_hip_ddh_plan_set_owner_rule(plan, last ? 1 : 0), "DDH owner rule");
        }

        template <typename Real>
        void DDHCore<Real>::set_wave_priority(bool high) const
        {
            ensure_plan();
            check_hip(cuddh_hip_ddh_plan_set_wave_priority(plan, high ? 1 : 0), "DDH wave priority");
        }

        template <typename Real>
        void DDHCore<Real>::ensure_assembly() const
        {
            if (_csr_off.size() > 0)
                return;
            const int N = mx_dof * n_domains;
            const int *gi = _gI.host_read();
            auto sizes = efem->sizes(MemorySpace::HOST);
            _gI_local.resize(N);
            int *loc = _gI_local.host_write();
            parallel_for(static_cast<std::size_t>(N), [&](std::size_t i0, std::size_t i1, int)
            {
                for (std::size_t i = i0; i < i1; ++i)
                    loc[i] = static_cast<int>(i);
            });
            _csr_off.resize(g_ndof + 1);
            int *off = _csr_off.host_write();
            std::fill(off, off + g_ndof + 1, 0);
            for (int s = 0; s < n_domains; ++s)
                for (int l = 0; l < sizes(s); ++l)
                    ++off[gi[l + static_cast<std::size_t>(mx_dof) * s] + 1];
            for (int g = 0; g < g_ndof; ++g)
                off[g + 1] += off[g];
            _csr_src.resize(off[g_ndof]);
            int *src = _csr_src.host_write();
            std::vector<int> fill(off, off + g_ndof);
            for (int s = 0; s < n_domains; ++s) // increasing subdomain: the order of a serial loop over the subdomains
                for (int l = 0; l < sizes(s); ++l)
                    src[fill[gi[l + static_cast<std::size_t>(mx_dof) * s]]++] = l + mx_dof * s;
            _x_local.resize(2 * N);
            _y_local.resize(2 * N);
        }

        template <typename Real>
        void DDHCore<Real>::solve(int d0, int d1, const double *x, double *y, bool zero_y, const Real *lambda, Real *update) const
        {
            solve_impl(nullptr, d0, d1, x, y, zero_y, lambda, update);
        }

        template <typename Real>
        void DDHCore<Real>::solve_listed(const int *d_domains, int n, const double *x, double *y, bool zero_y, const Real *lambda,
                                         Real *update) const
        {
            solve_impl(d_domains, 0, n, x, y, zero_y, lambda, update);
        }

        template <typename Real>
        void DDHCore<Real>::solve_impl(const int *d_list, int d0, int d1, const double *x, double *y, bool zero_y, const Real *lambda,
                                       Real *update) const
        {
            ensure_plan();
            auto run = [&](const double *xx, double *yy, bool zy)
            {
                int err;
                if constexpr (std::is_same_v<Real, float>)
                    err = d_list ? cuddh_hip_ddh_apply_list_f32(plan, d_list, d1, xx, yy, zy ? 1 : 0, lambda, update, stream())
                                 : cuddh_hip_ddh_apply_f32(plan, d0, d1, xx, yy, zy ? 1 : 0, lambda, update, stream());
                else
                    err = d_list ? cuddh_hip_ddh_apply_list_f64(plan, d_list, d1, xx, yy, zy ? 1 : 0, lambda, update, stream())
                                 : cuddh_hip_ddh_apply_f64(plan, d0, d1, xx, yy, zy ? 1 : 0, lambda, update, stream());
                check_hip(err, "DDH local solves");
            };
            if (!y)
            {
                run(x, nullptr, false);
                return;
            }
            // With a solution output the reference adds every subdomain's weighted values into y with atomics
            // (source/DDH.cpp:298-307), in whatever order the blocks finish.  Here the subdomains write into their own entries
            // (identity numbering) and a second kernel sums the copies of each global dof in increasing subdomain order:
            // postprocess is bitwise reproducible and equals a serial loop over the subdomains.
            // (footprint of this fixed-order assembly: two arrays of 2 * mx_dof * n_domains doubles, 0.54 GB at 1024^2 with n_basis 4,
            // kept for the lifetime of the object once a solution output was asked for; index arithmetic is 32-bit)
            if (2LL * mx_dof * n_domains > 2147483647LL)
                cuddh_error("DDH error: solution assembly needs 2 * mx_dof * n_domains < 2^31 (about 8192^2 elements at n_basis 4).");
            ensure_assembly();
            const int N = mx_dof * n_domains;
            const int *d_loc = _gI_local.device_read();
            double *xl = nullptr;
            if (x)
            {
                xl = _x_local.device_write();
                check_hip(cuddh_hip_gather_f64(N, _gI.device_read(), x, xl, stream()), "DDH forcing gather");
                check_hip(cuddh_hip_gather_f64(N, _gI.device_read(), x + g_ndof, xl + N, stream()), "DDH forcing gather");
            }
            double *yl = _y_local.device_write();
            check_hip(cuddh_hip_ddh_plan_set_vector_layout(plan, d_loc, N), "DDH local layout");
            try
            {
                run(xl, yl, true);
            }
            catch (...)
            {
                cuddh_hip_ddh_plan_set_vector_layout(plan, nullptr, 0);
                throw;
            }
            check_hip(cuddh_hip_ddh_plan_set_vector_layout(plan, nullptr, 0), "DDH layout reset");
            const int *off = _csr_off.device_read(), *src = _csr_src.device_read();
            check_hip(cuddh_hip_csr_sum_f64(g_ndof, off, src, yl, y, zero_y ? 0 : 1, stream()), "DDH solution assembly");
            check_hip(cuddh_hip_csr_sum_f64(g_ndof, off, src, yl + N, y + g_ndof, zero_y ? 0 : 1, stream()), "DDH solution assembly");
        }

        template <typename Real>
        void DDHCore<Real>::solve_listed(const int *d_domains, int n, const double *x, const Real *lambda, Real *update) const
        {
            solve_impl(d_domains, 0, n, x, nullptr, false, lambda, update);
        }

        template class DDHCore<float>;
        template class DDHCore<double>;
    } // namespace detail

    // ------------------------------------------------------------ DDH (fp32, reference precision)

    DDH::DDH(double omega, const double *h_a, const H1Space &fem, int nx, int ny) : core(omega, h_a, fem, nx, ny, 0) {}
    DDH::DDH(double omega, const double *h_a, const H1Space &fem, int nx, int ny, int kernel)
        : core(omega, h_a, fem, nx, ny, kernel)
    {
    }

    DDH::DDH(double omega, const double *h_a, const H1Space &fem, int nx, int ny, int kernel, int block)
        : core(omega, h_a, fem, nx, ny, kernel, block)
    {
    }

    DDH::DDH(double omega, const double *h_a, const H1Space &fem, int nx, int ny, int kernel, int block, const DDHTimeStep &time_step)
        : core(omega, h_a, fem, nx, ny, kernel, block, time_step)
    {
    }

    DDH::DDH(double omega, const double *h_a, const H1Space &fem, int nx, int ny, int kernel, int block, const DDHTimeStep &time_step,
             const DDHIntegrator &integrator)
        : core(omega, h_a, fem, nx, ny, kernel, block, time_step, integrator)
    {
    }

    DDH::DDH(from_labels_t tag, double omega, const double *h_a, const H1Space &fem, int n_domains, const int *labels, int kernel)
        : core(tag, omega, h_a, fem, n_domains, labels, kernel)
    {
    }

    DDH::DDH(from_labels_t tag, double omega, const double *h_a, const H1Space &fem, int n_domains, const int *labels, int kernel,
             const DDHTimeStep &time_step, const DDHIntegrator &integrator)
        : core(tag, omega, h_a, fem, n_domains, labels, kernel, time_step, integrator)
    {
    }

    void DDH::action(const float *x, float *y) const
    {
        core.solve(0, core.num_domains(), nullptr, nullptr, false, x, y);
        axpby(size(), 1.0f, x, -1.0f, y); // y = lambda - T lambda
    }

    void DDH::rhs(const double *f, float *b) const { core.solve(0, core.num_domains(), f, nullptr, false, nullptr, b); }

    void DDH::postprocess(const float *lambda, const double *f, double *u) const
    {
        core.solve(0, core.num_domains(), f, u, true, lambda, nullptr);
    }

    void DDH::local_traces(int d0, int d1, const double *f, const float *lambda, float *update) const
    {
        core.solve(d0, d1, f, nullptr, false, lambda, update);
    }

    void DDH::local_solution(int d0, int d1, const float *lambda, const double *f, double *u, bool zero_u) const
    {
        core.solve(d0, d1, f, u, zero_u, lambda, nullptr);
    }

    // ------------------------------------------------------------ DDH64 (fp64 parity mode)

    DDH64::DDH64(double omega, const double *h_a, const H1Space &fem, int nx, int ny, int kernel)
        : core(omega, h_a, fem, nx, ny, kernel)
    {
    }

    DDH64::DDH64(double omega, const double *h_a, const H1Space &fem, int nx, int ny, int kernel, int block)
        : core(omega, h_a, fem, nx, ny, kernel, block)
    {
    }

    DDH64::DDH64(double omega, const double *h_a, const H1Space &fem, int nx, int ny, int kernel, int block, const DDHTimeStep &time_step)
        : core(omega, h_a, fem, nx, ny, kernel, block, time_step)
    {
    }

    DDH64::DDH64(double omega, const double *h_a, const H1Space &fem, int nx, int ny, int kernel, int block, const DDHTimeStep &time_step,
                 const DDHIntegrator &integrator)
        : core(omega, h_a, fem, nx, ny, kernel, block, time_step, integrator)
    {
    }

    DDH64::DDH64(from_labels_t tag, double omega, const double *h_a, const H1Space &fem, int n_domains, const int *labels, int kernel)
        : core(tag, omega, h_a, fem, n_domains, labels, kernel)
    {
    }

    DDH64::DDH64(from_labels_t tag, double omega, const double *h_a, const H1Space &fem, int n_domains, const int *labels, int kernel,
                 const DDHTimeStep &time_step, const DDHIntegrator &integrator)
        : core(tag, omega, h_a, fem, n_domains, labels, kernel, time_step, integrator)
    {
    }

    void DDH64::action(const double *x, double *y) const
    {
        core.solve(0, core.num_domains(), nullptr, nullptr, false, x, y);
        axpby(size(), 1.0, x, -1.0, y);
    }

    void DDH64::action(double, const double *, double *) const
    {
        cuddh_error("DDH64::action(c, x, y) is not defined for the substructured operator.");
    }

    void DDH64::rhs(const double *f, double *b) const { core.solve(0, core.num_domains(), f, nullptr, false, nullptr, b); }

    void DDH64::postprocess(const double *lambda, const double *f, double *u) const
    {
        core.solve(0, core.num_domains(), f, u, true, lambda, nullptr);
    }

    void DDH64::local_traces(int d0, int d1, const double *f, const double *lambda, double *update) const
    {
        core.solve(d0, d1, f, nullptr, false, lambda, update);
    }

    void DDH64::local_solution(int d0, int d1, const double *lambda, const double *f, double *u, bool zero_u) const
    {
        core.solve(d0, d1, f, u, zero_u, lambda, nullptr);
    }
} // namespace cuddh
