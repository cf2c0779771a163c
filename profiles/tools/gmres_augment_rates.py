"""Two measurements for gmres(..., augment=k) (LGMRES), on one MI355X.

kernel   us of cuddh_hip_krylov_update_* (dx, x += dx and the partial sums of |dx|^2 in one launch) against the chain of k1 axpby
         launches on x that the unaugmented cycle ends with, k1 = 20 columns, alternating in the same run, device events around
         `inner` back-to-back repetitions.  Vector lengths: config 2's 256^2 and 1024^2 (fp64, 2 (3 nx + 1)^2) and the fp32 DDH
         trace vector of 512^2 (4 x 4-element subdomains: 4 * 2 (nx / 4) (nx / 4 - 1) * 13 entries).  Traffic in scalars: the
         update moves (k1 + 3) n, the chain 3 k1 n.
cycles   cd.gmres on the fp32 DDH operator with a = 1, GMRES(m), tol 1e-4, with and without augment: cycles and seconds (the
         solver's own clock, SolverOut.time) until the residual is at or below the plain run's final residual.
           stall     nx 512, omega = 16 pi, m 20, at most 39 cycles (GMRES(20) stalls at 0.097 there)
           example   the example's regime: five elements per wavelength (omega = 2 pi nx / 10), nx 32 and 48, m 20

  python profiles/tools/gmres_augment_rates.py [parts=kernel,stall,example] [augment=3] [reps=20]
"""
import ctypes as C
import math
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import cuddhelmholtz_amd as cd  # noqa: E402
from cuddhelmholtz_amd import _native as N  # noqa: E402

parts = (sys.argv[1] if len(sys.argv) > 1 else "kernel,stall,example").split(",")
augment = int(sys.argv[2]) if len(sys.argv) > 2 else 3
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
if not torch.cuda.is_available():
    sys.exit("gmres_augment_rates.py measures on the GPU: none is visible")
dev = torch.device("cuda:0")
cd.use_torch_stream()
K1 = 20


def kernel_case(name, n, dtype, inner):
    T = torch.float64 if dtype == "f64" else torch.float32
    item = 8 if dtype == "f64" else 4
    per16 = 16 // item
    ld = -(-n // per16) * per16
    g = torch.Generator(device=dev).manual_seed(1)
    V = torch.randn(K1 * ld, dtype=T, device=dev, generator=g)
    x0 = torch.randn(n, dtype=T, device=dev, generator=g)
    coef_h = np.linspace(-1.0, 1.0, K1)
    coef = torch.from_numpy(coef_h).to(T).to(dev)
    x, dx, part = x0.clone(), torch.empty_like(x0), torch.zeros(1024, dtype=T, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    upd, axp = getattr(N.lib, f"cuddh_hip_krylov_update_{dtype}"), getattr(N.lib, f"cuddh_hip_axpby_{dtype}")
    p = lambda t, k=0: C.c_void_p(t.data_ptr() + k * item)  # noqa: E731

    def update():
        N.check(upd(n, p(x), p(dx), p(V), ld, K1, None, 0, 0, p(coef), p(part), st), "krylov_update")

    def chain():
        for j in range(K1):
            N.check(axp(n, float(coef_h[j]), p(V, j * ld), 1.0, p(x), st), "axpby")

    # the two compute the same x (up to the order of the additions)
    x.copy_(x0)
    update()
    xu = x.clone()
    x.copy_(x0)
    chain()
    diff = float(torch.linalg.norm((xu - x).double()) / torch.linalg.norm(x.double()))
    times = {"update": [], "chain": []}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for rep in range(reps + 2):  # the first two passes warm up
        for what, f in (("update", update), ("chain", chain)):
            x.copy_(x0)
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(inner):
                f()
            ev[1].record()
            torch.cuda.synchronize()
            if rep >= 2:
                times[what].append(1e3 * ev[0].elapsed_time(ev[1]) / inner)
    u, c = statistics.median(times["update"]), statistics.median(times["chain"])
    bu, bc = (K1 + 3) * n * item, 3 * K1 * n * item
    print(f"KERNEL {name} {dtype} n={n} k1={K1}: update {u:.1f} us (min {min(times['update']):.1f}, max {max(times['update']):.1f}; "
          f"{bu / u / 1e6:.2f} TB/s of {K1 + 3} n scalars), axpby chain {c:.1f} us (min {min(times['chain']):.1f}, max {max(times['chain']):.1f}; "
          f"{bc / c / 1e6:.2f} TB/s of {3 * K1} n scalars), chain / update = {c / u:.2f} (traffic predicts {3 * K1 / (K1 + 3):.2f}); "
          f"|x_update - x_chain| / |x| = {diff:.1e}", flush=True)


def ddh_case(nx, omega):
    mesh = cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0)
    fem = cd.H1Space(mesh, cd.Basis(4))
    n = fem.size()
    F = cd.DDH(omega, np.ones(n), fem, nx, nx)
    f = torch.zeros(2 * n, dtype=torch.float64, device=dev)
    cd.linear_functional(fem, cd.GAUSSIANS, f[:n], param=omega)
    b = torch.zeros(F.size(), dtype=torch.float32, device=dev)
    F.rhs(f, b)
    return F, b, (mesh, fem)


def first_at_or_below(res, target):
    return next((i for i, r in enumerate(res) if r <= target), None)


def cycles_case(name, nx, omega, m, maxit, tol):
    F, b, keep = ddh_case(nx, omega)
    warm = torch.zeros_like(b)
    cd.gmres(F.size(), warm, F, b, m, 2, tol)  # warm-up: one cycle
    outs = {}
    for aug in (0, augment):
        x = torch.zeros_like(b)
        torch.cuda.synchronize()
        outs[aug] = out = cd.gmres(F.size(), x, F, b, m, maxit, tol, augment=aug)
        rel = [r / out.res_norm[0] for r in out.res_norm]
        print(f"CYCLES {name} nx={nx} n={F.size()} GMRES({m}) augment={aug}: success={out.success} cycles={out.num_iter} matvecs={out.num_matvec} "
              f"seconds={out.time[-1]:.3f} rel_res={rel[-1]:.4e}", flush=True)
        print(f"  residuals augment={aug}: " + " ".join(f"{r:.4e}" for r in rel), flush=True)
    plain, aug = outs[0], outs[augment]
    target = plain.res_norm[-1]
    i = first_at_or_below(aug.res_norm, target)
    j = first_at_or_below(plain.res_norm, target)
    if i is None:
        print(f"SUMMARY {name} nx={nx}: the augmented run never reaches the plain run's final residual {target / plain.res_norm[0]:.4e} "
              f"(its own final: {aug.res_norm[-1] / aug.res_norm[0]:.4e} after {aug.num_iter} cycles, {aug.time[-1]:.3f} s; plain {plain.time[-1]:.3f} s)", flush=True)
    else:
        print(f"SUMMARY {name} nx={nx}: to the plain run's final residual {target / plain.res_norm[0]:.4e}: plain {j} cycles, {plain.time[j]:.3f} s, "
              f"{plain.num_matvec} matvecs in all; augment={augment} {i} cycles, {aug.time[i]:.3f} s (whole run: {aug.num_iter} cycles, {aug.num_matvec} matvecs, "
              f"{aug.time[-1]:.3f} s, final {aug.res_norm[-1] / aug.res_norm[0]:.4e})", flush=True)
    del keep


if "kernel" in parts:
    kernel_case("config 2, 256^2", 2 * (3 * 256 + 1) ** 2, "f64", 20)
    kernel_case("config 2, 1024^2", 2 * (3 * 1024 + 1) ** 2, "f64", 5)
    kernel_case("fp32 DDH traces, 512^2", 4 * 2 * 128 * 127 * 13, "f32", 20)
if "stall" in parts:
    cycles_case("stall", 512, 16 * math.pi, 20, 40, 1e-4)
if "example" in parts:
    for nx in (32, 48):
        cycles_case("example", nx, 2 * math.pi * nx / 10, 20, 100, 1e-4)
