// Native C++ driver for the whole-domain WaveHoltz solver (csrc/include/cuddh/waveholtz.hpp), in ddh_solve's style:
//   waveholtz_solve [nx=128] [n_basis=4] [omega_over_pi=25.6] [gmres_m=20] [maxit=100] [tol=1e-4] [out_dir=-]
//   options, anywhere on the line: --integrator rk2|rk4 --coarsen N (rk2 on the mesh grid is the default; rk4 marches
//   ceil(nt / N) steps, N in [1, 16], 4 unless given), --time-ratio R|coefficient (the period's step count times R in [1, 256], or
//   the ratio the coefficient asks for; 1 is the default), --stiffness gauss|lobatto (the sweep's quadrature, WaveHoltzOptions;
//   gauss is the default), --sweep operator|lattice (lattice: one launch per sweep on the Gauss-Lobatto lattice; it implies
//   --stiffness lobatto and refuses --stiffness gauss), --precision f64|f32 (f32: the lattice sweeps in fp32, for tolerances around
//   1e-4; it goes with --sweep lattice only), --launch sweep|pair (pair: two lattice sweeps per launch, the same march bit for bit;
//   it goes with --sweep lattice only), --coefficient one|disk (a == 1, the default, or the examples' disk of a = 0.2, projected as in
//   ddh_solve), --void i0 j0 i1 j1 (any number of times: the cells i0 <= i < i1, j0 <= j < j1 of the nx x nx grid are left out, a
//   sound-hard or absorbing obstacle; --sweep lattice then runs the sweeps with missing cells and refuses --launch pair; every
//   boundary edge, the obstacle's walls included, is absorbing), --inclusion i0 j0 i1 j1 beta (any number of times: the stiffness
//   coefficient beta > 0 on the cells i0 <= i < i1, j0 <= j < j1 and 1 elsewhere, -div(beta grad U) - w^2 a^2 U = f; it goes with
//   --sweep lattice only, refuses --launch pair and composes with --void, whose cells take no value), --residuals (one more line: GMRES's residual history).
// The load is the examples' pair of Gaussians in the real part and 0.1 (3 x^2 - 2 x y + y + 1) in the imaginary part.
// Writes <out_dir>/xy.0000 and <out_dir>/waveholtz.0000 (raw fp64; "-": nothing) and prints one summary line.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <string>
#include <vector>

#include "cuddh.hpp"
#include "cuddh_hip.h"
#include "examples.hpp"

using namespace cuddh;

int main(int argc_all, char **argv_all)
{
    std::string integrator = "rk2", time_ratio = "1", stiffness = "", coefficient = "one", sweep = "operator", precision = "f64", launch = "sweep";
    int coarsen = 0; // 0: not given
    bool residuals = false;
    std::vector<int> voids; // four per --void
    std::vector<int> inclusions;  // four per --inclusion
    std::vector<double> betas;    // one per --inclusion
    std::vector<char *> args;
    for (int i = 0; i < argc_all; ++i)
    {
        const std::string arg = argv_all[i];
        if (arg == "--integrator" && i + 1 < argc_all)
            integrator = argv_all[++i];
        else if (arg == "--coarsen" && i + 1 < argc_all)
            coarsen = std::atoi(argv_all[++i]);
        else if (arg == "--time-ratio" && i + 1 < argc_all)
            time_ratio = argv_all[++i];
        else if (arg == "--stiffness" && i + 1 < argc_all)
            stiffness = argv_all[++i];
        else if (arg == "--sweep" && i + 1 < argc_all)
            sweep = argv_all[++i];
        else if (arg == "--precision" && i + 1 < argc_all)
            precision = argv_all[++i];
        else if (arg == "--launch" && i + 1 < argc_all)
            launch = argv_all[++i];
        else if (arg == "--coefficient" && i + 1 < argc_all)
            coefficient = argv_all[++i];
        else if (arg == "--void" && i + 4 < argc_all)
        {
            for (int k = 0; k < 4; ++k)
                voids.push_back(std::atoi(argv_all[++i]));
        }
        else if (arg == "--void")
        {
            std::cerr << "waveholtz_solve: --void takes four cell indices: i0 j0 i1 j1" << std::endl;
            return 2;
        }
        else if (arg == "--inclusion" && i + 5 < argc_all)
        {
            for (int k = 0; k < 4; ++k)
                inclusions.push_back(std::atoi(argv_all[++i]));
            betas.push_back(std::atof(argv_all[++i]));
        }
        else if (arg == "--inclusion")
        {
            std::cerr << "waveholtz_solve: --inclusion takes four cell indices and a coefficient: i0 j0 i1 j1 beta" << std::endl;
            return 2;
        }
        else if (arg == "--residuals")
            residuals = true;
        else
            args.push_back(argv_all[i]);
    }
    if (integrator != "rk2" && integrator != "rk4")
    {
        std::cerr << "waveholtz_solve: --integrator takes rk2 or rk4, not " << integrator << std::endl;
        return 2;
    }
    if (coarsen == 0)
        coarsen = integrator == "rk4" ? 4 : 1;
    if (coarsen < 1 || coarsen > DDHIntegrator::max_coarsen || (integrator == "rk2" && coarsen != 1))
    {
        std::cerr << "waveholtz_solve: --coarsen takes 1 to " << DDHIntegrator::max_coarsen << " with --integrator rk4, and 1 with rk2" << std::endl;
        return 2;
    }
    const int ratio = time_ratio == "coefficient" ? WaveHoltzOptions::from_coefficient : std::atoi(time_ratio.c_str());
    if (time_ratio != "coefficient" && (ratio < 1 || ratio > DDHTimeStep::max_ratio))
    {
        std::cerr << "waveholtz_solve: --time-ratio takes coefficient or 1 to " << DDHTimeStep::max_ratio << ", not " << time_ratio << std::endl;
        return 2;
    }
    if (sweep != "operator" && sweep != "lattice")
    {
        std::cerr << "waveholtz_solve: --sweep takes operator or lattice, not " << sweep << std::endl;
        return 2;
    }
    if (stiffness.empty())
        stiffness = sweep == "lattice" ? "lobatto" : "gauss";
    if (sweep == "lattice" && stiffness != "lobatto")
    {
        std::cerr << "waveholtz_solve: --sweep lattice is the collocated stiffness: it goes with --stiffness lobatto only" << std::endl;
        return 2;
    }
    if (stiffness != "gauss" && stiffness != "lobatto")
    {
        std::cerr << "waveholtz_solve: --stiffness takes gauss or lobatto, not " << stiffness << std::endl;
        return 2;
    }
    if (precision != "f64" && precision != "f32")
    {
        std::cerr << "waveholtz_solve: --precision takes f64 or f32, not " << precision << std::endl;
        return 2;
    }
    if (precision == "f32" && sweep != "lattice")
    {
        std::cerr << "waveholtz_solve: --precision f32 is the lattice sweeps in fp32: it goes with --sweep lattice only" << std::endl;
        return 2;
    }
    if (launch != "sweep" && launch != "pair")
    {
        std::cerr << "waveholtz_solve: --launch takes sweep or pair, not " << launch << std::endl;
        return 2;
    }
    if (launch == "pair" && sweep != "lattice")
    {
        std::cerr << "waveholtz_solve: --launch pair is two lattice sweeps per launch: it goes with --sweep lattice only" << std::endl;
        return 2;
    }
    if (!voids.empty() && launch == "pair")
    {
        std::cerr << "waveholtz_solve: --launch pair has no form for a grid with missing cells yet: it does not go with --void" << std::endl;
        return 2;
    }
    if (!betas.empty() && sweep != "lattice")
    {
        std::cerr << "waveholtz_solve: --inclusion is a per-cell stiffness of the lattice sweeps: it goes with --sweep lattice only" << std::endl;
        return 2;
    }
    if (!betas.empty() && launch == "pair")
    {
        std::cerr << "waveholtz_solve: --launch pair has no form for a per-cell stiffness: it does not go with --inclusion" << std::endl;
        return 2;
    }
    if (coefficient != "one" && coefficient != "disk")
    {
        std::cerr << "waveholtz_solve: --coefficient takes one or disk, not " << coefficient << std::endl;
        return 2;
    }
    const int argc = static_cast<int>(args.size());
    char **argv = args.data();
    const int nx = argc > 1 ? std::atoi(argv[1]) : 128;
    const int nb = argc > 2 ? std::atoi(argv[2]) : 4;
    const double omega = M_PI * (argc > 3 ? std::atof(argv[3]) : 25.6);
    const int m = argc > 4 ? std::atoi(argv[4]) : 20;
    const int maxit = argc > 5 ? std::atoi(argv[5]) : 100;
    const double tol = argc > 6 ? std::atof(argv[6]) : 1e-4;
    const std::string out_dir = argc > 7 ? argv[7] : "-";

    std::vector<unsigned char> present(static_cast<std::size_t>(std::max(nx, 1)) * std::max(nx, 1), 1);
    for (std::size_t k = 0; k + 3 < voids.size(); k += 4)
    {
        const int i0 = voids[k], j0 = voids[k + 1], i1 = voids[k + 2], j1 = voids[k + 3];
        if (i0 < 0 || j0 < 0 || i1 > nx || j1 > nx || i0 >= i1 || j0 >= j1)
        {
            std::cerr << "waveholtz_solve: --void " << i0 << " " << j0 << " " << i1 << " " << j1 << " is no box of cells of the " << nx << " x " << nx
                      << " grid" << std::endl;
            return 2;
        }
        for (int j = j0; j < j1; ++j)
            for (int i = i0; i < i1; ++i)
                present[i + static_cast<std::size_t>(nx) * j] = 0;
    }
    std::vector<double> cell_beta(betas.empty() ? 0 : present.size(), 1.0);
    for (std::size_t k = 0; k < betas.size(); ++k)
    {
        const int i0 = inclusions[4 * k], j0 = inclusions[4 * k + 1], i1 = inclusions[4 * k + 2], j1 = inclusions[4 * k + 3];
        if (i0 < 0 || j0 < 0 || i1 > nx || j1 > nx || i0 >= i1 || j0 >= j1 || !(betas[k] > 0.0) || !std::isfinite(betas[k]))
        {
            std::cerr << "waveholtz_solve: --inclusion " << i0 << " " << j0 << " " << i1 << " " << j1 << " " << betas[k]
                      << " is no box of cells of the " << nx << " x " << nx << " grid with a finite positive coefficient" << std::endl;
            return 2;
        }
        for (int j = j0; j < j1; ++j)
            for (int i = i0; i < i1; ++i)
                cell_beta[i + static_cast<std::size_t>(nx) * j] = betas[k];
    }
    // element order: the present cells, ascending
    std::vector<double> beta;
    for (std::size_t c = 0; c < cell_beta.size(); ++c)
        if (present[c])
            beta.push_back(cell_beta[c]);
    Mesh2D mesh = voids.empty() ? Mesh2D::uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0) : grid_cells(nx, -1.0, 1.0, nx, -1.0, 1.0, present.data());
    Basis basis(nb);
    H1Space fem(mesh, basis);
    const int ndof = fem.size(), N = 2 * ndof;

    host_device_dvec U(N), z(N), f(N), b(N), a(ndof);
    double *d_U = U.device_write(), *d_z = z.device_write(), *d_f = f.device_write(), *d_b = b.device_write(), *d_a = a.device_write();

    LinearFunctional l(fem);
    l.action([=] __device__(const double X[2]) -> double
    {
        const double s = omega * omega;
        const double r0 = (X[0] + 0.5) * (X[0] + 0.5) + X[1] * X[1];
        const double r1 = (X[0] - 0.5) * (X[0] - 0.5) + (X[1] + 0.5) * (X[1] + 0.5);
        return s / M_PI * (exp(-s * r0) + exp(-s * r1));
    }, d_f);
    l.action([] __device__(const double X[2]) -> double { return 0.1 * (3.0 * X[0] * X[0] - 2.0 * X[0] * X[1] + X[1] + 1.0); }, d_f + ndof);
    if (coefficient == "disk")
    {
        DiagInvMassMatrix mi(fem);
        l.action([] __device__(const double X[2]) -> double { return (X[0] * X[0] + X[1] * X[1] < 0.0625) ? 0.2 : 1.0; }, d_a);
        mi.action(d_a, d_a);
    }
    else
        ones(ndof, d_a);

    WaveHoltzOptions opt;
    opt.integrator = {integrator == "rk4" ? DDHIntegrator::rk4 : DDHIntegrator::rk2, coarsen};
    opt.time_ratio = ratio;
    opt.stiffness = stiffness == "lobatto" ? WaveHoltzOptions::lobatto : WaveHoltzOptions::gauss;
    opt.sweep = sweep == "lattice" ? WaveHoltzOptions::lattice : WaveHoltzOptions::operator_kernels;
    opt.precision = precision == "f32" ? WaveHoltzOptions::f32 : WaveHoltzOptions::f64;
    opt.launch = launch == "pair" ? WaveHoltzOptions::per_pair : WaveHoltzOptions::per_sweep;
    if (!betas.empty())
        opt.h_cell_stiffness = beta.data();
    WaveHoltz W(omega, a.host_read(), fem, opt);

    // wall time of each phase with a device sync at both ends, as ddh_solve
    using clk = std::chrono::steady_clock;
    auto seconds_since = [](clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); };
    auto sync = [] { detail::check_hip(cuddh_hip_stream_sync(stream()), "sync"); };
    sync();
    auto t = clk::now();
    W.rhs(d_f, d_b);
    sync();
    const double t_rhs = seconds_since(t);
    t = clk::now();
    solver_out out = gmres(N, d_z, &W, d_b, m, maxit, tol);
    sync();
    const double t_gmres = seconds_since(t);
    W.solution(d_z, d_U);
    sync();
    const double *h_U = U.host_read();

    if (out_dir != "-")
    {
        to_file(out_dir + "/xy.0000", N, fem.physical_coordinates(MemorySpace::HOST));
        to_file(out_dir + "/waveholtz.0000", N, h_U);
    }
    double unorm = 0.0;
    for (int i = 0; i < N; ++i)
        unorm += h_U[i] * h_U[i];
    const double ms_per_period = out.num_matvec > 0 ? 1e3 * t_gmres / out.num_matvec : 0.0;
    std::cout << "waveholtz_solve nx=" << nx << " nb=" << nb << " omega/pi=" << omega / M_PI << " ndof=" << ndof << " integrator=" << integrator
              << " coarsen=" << coarsen << " ratio=" << W.time_ratio() << " stiffness=" << stiffness << " sweep=" << sweep << " precision=" << precision << " launch=" << launch << " coefficient=" << coefficient
              << (voids.empty() ? "" : " cells=" + std::to_string(mesh.n_elem()))
              << " nt=" << W.num_steps() << " sweeps_per_period=" << W.sweeps_per_period() << " success=" << out.success
              << " num_iter=" << out.num_iter << " num_matvec=" << out.num_matvec << " rel_res=" << out.res_norm.back() / out.res_norm.front()
              << " |u|=" << std::sqrt(unorm) << " t_rhs=" << t_rhs << " t_gmres=" << t_gmres << " ms_per_period=" << ms_per_period
              << " us_per_sweep=" << 1e3 * ms_per_period / W.sweeps_per_period() << " kernel=\"" << W.stiffness_kernel() << "\"" << std::endl;
    if (residuals)
    {
        std::cout << "waveholtz_solve residuals:";
        for (const double r : out.res_norm)
            std::cout << " " << r / out.res_norm.front();
        std::cout << std::endl;
    }
    return 0;
}
