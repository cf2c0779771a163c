// Native C++ driver for the DDH path, written against csrc/include/cuddh.hpp (the same API the reference's
// examples/DDH.cpp uses), with a command line instead of compile-time constants:
//   ddh_solve [nx=128] [n_basis=4] [omega_over_pi=25.6] [gmres_m=20] [maxit=100] [tol=1e-4] [out_dir=solution] [devices=0] [force_rccl=0]
//   options, anywhere on the line: --time-step mesh|coefficient (DDHTimeStep: where the local solves take their time step from;
//   mesh is the default, the reference's; single-process path only), --integrator rk2|rk4 --coarsen N (DDHIntegrator: rk2 on
//   the mesh grid is the default; rk4 marches ceil(nt / N) steps, N in [1, 16], 4 unless given; single-process path only),
//   --residuals (one more line: GMRES's residual history), --orth mgs|cgs2 (the orthogonalisation of the Arnoldi step, krylov.hpp;
//   mgs is the default, the reference's; both paths; the summary line names it when it is not mgs), --augment K (LGMRES: the last
//   K corrections augment every restart cycle, krylov.hpp GmresOptions; 0 <= K < m, 0 is the default; single-process path only;
//   the summary line names it when it is not 0), --block N --kernel K (the DDH constructor's block and kernel: N x N elements
//   per subdomain, 0 the reference's 16 / n_basis; K as cuddh_hip_ddh_plan_create numbers them, 0 auto; single-process path
//   only; n_basis 5 needs --block 4 wherever 3 does not divide nx, and then runs kernel 12 where auto or K = 12 picks it, and K = 13
//   (the same local solves, on per-subdomain time grids too) together with --time-step coefficient; the
//   summary line names block and kernel when either is given), --arithmetic real|complex (krylov.hpp Arithmetic: complex runs
//   GMRES over the complex numbers on the trace vectors [lambda; mu]; real is the default; needs --orth mgs and --augment 0;
//   single-process path only; the summary line names it when it is complex), --chain-order auto|pinned|paired (DDHCore::set_chain_order:
//   the summation order of kernel 5's element-lane form; auto is the default; single-process path only; an order the plan cannot
//   take ends the run; the summary line names the order asked for and the one in effect when it is not auto),
//   --forcing auto|every|first (DDHCore::set_forcing: where that form's march applies the trace sources, in every WaveHoltz pass
//   or in the first only; the same rules and the same note as --chain-order), --march auto|plain|scaled (DDHCore::set_march: how
//   the march of forcing "first" carries the velocity, as it is or scaled with its midpoint update folded into the sweep; the
//   same rules and the same note), --head auto|multiplied|carried (DDHCore::set_head: what the scaled march carries as the
//   velocity, q / (2 hm) multiplied by the first chain's head coefficient in every step, or that product itself; the same rules
//   and the same note), --assembly auto|dpp|fetched (DDHCore::set_assembly: how head "carried" forms the neighbour sums of its
//   sweeps, with DPP on the vector pipe or fetched both ways over the LDS pipe, the same bits; the same rules and the same note)
// Writes <out_dir>/xy.0000 and <out_dir>/ddh.0000 (raw fp64, like the reference) and prints one summary line.
// devices >= 1: the same solve through cuddh::ddh_solve_multi_gpu (multigpu.hpp): subdomains sharded over that many GPUs of
// this process, RCCL neighbour exchange; devices = 1 with force_rccl = 1 runs the communicator path on a one-GPU box;
// force_rccl = 2 is the loopback test transport (the ranks share device 0, no RCCL); + 4 selects the split schedule.
#include <chrono>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "cuddh.hpp"
#include "cuddh_hip.h"
#include "examples.hpp"

using namespace cuddh;

int main(int argc_all, char **argv_all)
{
    // options out, positional arguments stay
    std::string time_step = "mesh", integrator = "rk2", orth_name = "mgs", arithmetic = "real", chain_order = "auto", forcing = "auto", march = "auto", head = "auto", assembly = "auto";
    int coarsen = 0; // 0: not given
    int augment = 0, block = 0, kernel = 0;
    bool residuals = false, block_given = false;
    std::vector<char *> args;
    for (int i = 0; i < argc_all; ++i)
    {
        const std::string arg = argv_all[i];
        if (arg == "--time-step" && i + 1 < argc_all)
            time_step = argv_all[++i];
        else if (arg == "--integrator" && i + 1 < argc_all)
            integrator = argv_all[++i];
        else if (arg == "--coarsen" && i + 1 < argc_all)
            coarsen = std::atoi(argv_all[++i]);
        else if (arg == "--orth" && i + 1 < argc_all)
            orth_name = argv_all[++i];
        else if (arg == "--augment" && i + 1 < argc_all)
            augment = std::atoi(argv_all[++i]);
        else if (arg == "--arithmetic" && i + 1 < argc_all)
            arithmetic = argv_all[++i];
        else if (arg == "--chain-order" && i + 1 < argc_all)
            chain_order = argv_all[++i];
        else if (arg == "--forcing" && i + 1 < argc_all)
            forcing = argv_all[++i];
        else if (arg == "--march" && i + 1 < argc_all)
            march = argv_all[++i];
        else if (arg == "--head" && i + 1 < argc_all)
            head = argv_all[++i];
        else if (arg == "--assembly" && i + 1 < argc_all)
            assembly = argv_all[++i];
        else if (arg == "--block" && i + 1 < argc_all)
        {
            block = std::atoi(argv_all[++i]);
            block_given = true;
        }
        else if (arg == "--kernel" && i + 1 < argc_all)
        {
            kernel = std::atoi(argv_all[++i]);
            block_given = true;
        }
        else if (arg == "--residuals")
            residuals = true;
        else
            args.push_back(argv_all[i]);
    }
    if (time_step != "mesh" && time_step != "coefficient")
    {
        std::cerr << "ddh_solve: --time-step takes mesh or coefficient, not " << time_step << std::endl;
        return 2;
    }
    if (integrator != "rk2" && integrator != "rk4")
    {
        std::cerr << "ddh_solve: --integrator takes rk2 or rk4, not " << integrator << std::endl;
        return 2;
    }
    if (orth_name != "mgs" && orth_name != "cgs2")
    {
        std::cerr << "ddh_solve: --orth takes mgs or cgs2, not " << orth_name << std::endl;
        return 2;
    }
    const Orthogonalization orth = orth_name == "cgs2" ? Orthogonalization::cgs2 : Orthogonalization::mgs;
    const std::string orth_note = orth_name == "mgs" ? "" : " orth=" + orth_name;
    if (coarsen == 0)
        coarsen = integrator == "rk4" ? 4 : 1;
    if (coarsen < 1 || coarsen > DDHIntegrator::max_coarsen || (integrator == "rk2" && coarsen != 1))
    {
        std::cerr << "ddh_solve: --coarsen takes 1 to " << DDHIntegrator::max_coarsen << " with --integrator rk4, and 1 with rk2" << std::endl;
        return 2;
    }
    const int argc = static_cast<int>(args.size());
    char **argv = args.data();
    const int nx = argc > 1 ? std::atoi(argv[1]) : 128;
    const int nb = argc > 2 ? std::atoi(argv[2]) : 4;
    const double omega = M_PI * (argc > 3 ? std::atof(argv[3]) : 25.6);
    const int m = argc > 4 ? std::atoi(argv[4]) : 20;
    const int maxit = argc > 5 ? std::atoi(argv[5]) : 100;
    const float tol = argc > 6 ? static_cast<float>(std::atof(argv[6])) : 1e-4f;
    const std::string out_dir = argc > 7 ? argv[7] : "solution";
    const int devices = argc > 8 ? std::atoi(argv[8]) : 0;
    const int force_rccl = argc > 9 ? std::atoi(argv[9]) : 0; // transport: 0 auto, 1 RCCL also for one rank, 2 loopback (ranks share device 0)
    if (augment < 0 || (augment > 0 && augment >= m) || (augment > 0 && devices >= 1))
    {
        std::cerr << "ddh_solve: --augment takes 0 to m - 1 = " << m - 1 << " on the single-process path, not " << augment << std::endl;
        return 2;
    }
    const std::string aug_note = augment == 0 ? "" : " augment=" + std::to_string(augment);
    if (arithmetic != "real" && arithmetic != "complex")
    {
        std::cerr << "ddh_solve: --arithmetic takes real or complex, not " << arithmetic << std::endl;
        return 2;
    }
    if (arithmetic == "complex" && (orth_name != "mgs" || augment != 0 || devices >= 1))
    {
        std::cerr << "ddh_solve: --arithmetic complex needs --orth mgs and --augment 0 on the single-process path" << std::endl;
        return 2;
    }
    const std::string arith_note = arithmetic == "real" ? "" : " arithmetic=" + arithmetic;
    if ((chain_order != "auto" && chain_order != "pinned" && chain_order != "paired") || (chain_order != "auto" && devices >= 1))
    {
        std::cerr << "ddh_solve: --chain-order takes auto, pinned or paired on the single-process path, not " << chain_order << std::endl;
        return 2;
    }
    if ((forcing != "auto" && forcing != "every" && forcing != "first") || (forcing != "auto" && devices >= 1))
    {
        std::cerr << "ddh_solve: --forcing takes auto, every or first on the single-process path, not " << forcing << std::endl;
        return 2;
    }
    if ((march != "auto" && march != "plain" && march != "scaled") || (march != "auto" && devices >= 1))
    {
        std::cerr << "ddh_solve: --march takes auto, plain or scaled on the single-process path, not " << march << std::endl;
        return 2;
    }
    if ((head != "auto" && head != "multiplied" && head != "carried") || (head != "auto" && devices >= 1))
    {
        std::cerr << "ddh_solve: --head takes auto, multiplied or carried on the single-process path, not " << head << std::endl;
        return 2;
    }
    if ((assembly != "auto" && assembly != "dpp" && assembly != "fetched") || (assembly != "auto" && devices >= 1))
    {
        std::cerr << "ddh_solve: --assembly takes auto, dpp or fetched on the single-process path, not " << assembly << std::endl;
        return 2;
    }
    if (block < 0 || kernel < 0 || (block_given && devices >= 1))
    {
        std::cerr << "ddh_solve: --block and --kernel take non-negative integers on the single-process path" << std::endl;
        return 2;
    }

    Mesh2D mesh = Mesh2D::uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0);
    Basis basis(nb);
    H1Space fem(mesh, basis);
    const int ndof = fem.size(), N = 2 * ndof;

    host_device_dvec U(N), b(N), a(ndof);
    double *d_U = U.device_write(), *d_b = b.device_write(), *d_a = a.device_write();

    LinearFunctional l(fem);
    DiagInvMassMatrix mi(fem);
    l.action([=] __device__(const double X[2]) -> double
    {
        const double s = omega * omega;
        const double r0 = (X[0] + 0.5) * (X[0] + 0.5) + X[1] * X[1];
        const double r1 = (X[0] - 0.5) * (X[0] - 0.5) + (X[1] + 0.5) * (X[1] + 0.5);
        return s / M_PI * (exp(-s * r0) + exp(-s * r1));
    }, d_b);
    l.action([] __device__(const double X[2]) -> double { return (X[0] * X[0] + X[1] * X[1] < 0.0625) ? 0.2 : 1.0; }, d_a);
    mi.action(d_a, d_a);

    if (devices >= 1)
    {
        if (time_step != "mesh")
        {
            std::cerr << "ddh_solve: --time-step " << time_step << " is not passed through the multi-GPU path" << std::endl;
            return 2;
        }
        if (integrator != "rk2")
        {
            std::cerr << "ddh_solve: --integrator " << integrator << " is not passed through the multi-GPU path" << std::endl;
            return 2;
        }
        std::vector<double> h_u(N);
        const multi_gpu_result r = ddh_solve_multi_gpu(nx, nb, omega, a.host_read(), b.host_read(), h_u.data(), devices, m, maxit, tol, force_rccl & 3,
                                                       (force_rccl & 4) != 0, (force_rccl >> 8) & 0xFF, (force_rccl >> 16) & 0xFF, orth);
        if (out_dir != "-")
        {
            to_file(out_dir + "/xy.0000", N, fem.physical_coordinates(MemorySpace::HOST));
            to_file(out_dir + "/ddh.0000", N, h_u.data());
        }
        double unorm = 0.0;
        for (int i = 0; i < N; ++i)
            unorm += h_u[i] * h_u[i];
        std::cout << "ddh_solve nx=" << nx << " nb=" << nb << " omega/pi=" << omega / M_PI << " ndof=" << ndof << " devices=" << r.world
                  << " rccl=" << r.used_rccl << " success=" << r.gmres.success << " num_iter=" << r.gmres.num_iter
                  << " num_matvec=" << r.gmres.num_matvec << " rel_res=" << r.gmres.res_norm.back() / r.gmres.res_norm.front()
                  << " |u|=" << std::sqrt(unorm) << " t_setup=" << r.t_setup << " t_rhs=" << r.t_rhs << " t_gmres=" << r.t_gmres
                  << " t_postprocess=" << r.t_postprocess << " sent_bytes_per_action_rank0=" << r.bytes_sent_per_action_rank0
                  << " DoF*iter/s=" << 2.0 * ndof * r.gmres.num_matvec / r.t_gmres << orth_note << std::endl;
        return 0;
    }

    const DDHTimeStep ts = time_step == "mesh" ? DDHTimeStep::from_mesh() : DDHTimeStep::from_coefficient();
    std::unique_ptr<DDH> ddh(integrator == "rk4"   ? new DDH(omega, a.host_read(), fem, nx, nx, kernel, block, ts, DDHIntegrator::rk4_on(coarsen))
                             : time_step != "mesh" ? new DDH(omega, a.host_read(), fem, nx, nx, kernel, block, ts)
                             : block_given         ? new DDH(omega, a.host_read(), fem, nx, nx, kernel, block)
                                                   : new DDH(omega, a.host_read(), fem, nx, nx));
    DDH &F = *ddh;
    if (chain_order != "auto")
        F.internals().set_chain_order(chain_order == "paired" ? 2 : 1);
    const std::string chain_note = chain_order == "auto" ? "" : " chain_order=" + chain_order + " in_effect=" + std::to_string(F.internals().chain_order());
    if (forcing != "auto")
        F.internals().set_forcing(forcing == "first" ? 2 : 1);
    const std::string forcing_note = forcing == "auto" ? "" : " forcing=" + forcing + " in_effect=" + std::to_string(F.internals().forcing());
    if (march != "auto")
        F.internals().set_march(march == "scaled" ? 2 : 1);
    const std::string march_note = march == "auto" ? "" : " march=" + march + " in_effect=" + std::to_string(F.internals().march());
    if (head != "auto")
        F.internals().set_head(head == "carried" ? 2 : 1);
    if (assembly != "auto")
        F.internals().set_assembly(assembly == "fetched" ? 2 : 1);
    const std::string assembly_note = assembly == "auto" ? "" : " assembly=" + assembly + " in_effect=" + std::to_string(F.internals().assembly());
    const std::string head_note = head == "auto" ? "" : " head=" + head + " in_effect=" + std::to_string(F.internals().head());
    const int n_lambda = F.size();
    HostDeviceArray<float> L(n_lambda), Y(n_lambda);
    float *d_L = L.device_write(), *d_Y = Y.device_write();

    // timing as SURVEY 8d defines the solver metric: wall time of the gmres() call with a device sync at both ends;
    // rhs and postprocess reported separately
    using clk = std::chrono::steady_clock;
    auto seconds_since = [](clk::time_point t) { return std::chrono::duration<double>(clk::now() - t).count(); };
    auto sync = [] { detail::check_hip(cuddh_hip_stream_sync(stream()), "sync"); };
    sync();
    auto t = clk::now();
    F.rhs(d_b, d_Y);
    sync();
    const double t_rhs = seconds_since(t);
    t = clk::now();
    solver_out out = gmres(n_lambda, d_L, &F, d_Y, m, maxit, tol, 0, 6 * 60 * 60, GmresOptions{orth, augment, arithmetic == "complex" ? Arithmetic::complex : Arithmetic::real});
    sync();
    const double t_gmres = seconds_since(t);
    t = clk::now();
    F.postprocess(d_L, d_b, d_U);
    sync();
    const double t_post = seconds_since(t);
    const double *h_U = U.host_read();
    const std::string block_note = block_given ? " block=" + std::to_string(block) + " kernel=" + std::to_string(F.internals().kernel_kind()) : "";

    if (out_dir != "-")
    {
        to_file(out_dir + "/xy.0000", N, fem.physical_coordinates(MemorySpace::HOST));
        to_file(out_dir + "/ddh.0000", N, h_U);
    }
    double unorm = 0.0;
    for (int i = 0; i < N; ++i)
        unorm += h_U[i] * h_U[i];
    std::cout << "ddh_solve nx=" << nx << " nb=" << nb << " omega/pi=" << omega / M_PI << " ndof=" << ndof << " n_lambda=" << n_lambda
              << " success=" << out.success << " num_iter=" << out.num_iter << " num_matvec=" << out.num_matvec
              << " rel_res=" << out.res_norm.back() / out.res_norm.front() << " |u|=" << std::sqrt(unorm) << " t_rhs=" << t_rhs
              << " t_gmres=" << t_gmres << " t_postprocess=" << t_post
              << " DoF*iter/s=" << 2.0 * ndof * out.num_matvec / t_gmres << orth_note << aug_note << arith_note << block_note << chain_note << forcing_note << march_note << head_note << assembly_note << std::endl;
    if (residuals)
    {
        std::cout << "ddh_solve time_step=" << time_step << " residuals:";
        for (const double r : out.res_norm)
            std::cout << " " << r / out.res_norm.front();
        std::cout << std::endl;
    }
    return 0;
}
