"""Measurements for gmres(..., arithmetic="complex") against the real iteration, on one MI355X.

step     us per Arnoldi step (operator application + Gram-Schmidt chain + normalisation + the host's share), complex against real,
         GMRES(20), tol 0, `cycles` full cycles after one warm-up cycle, alternating in the same run; the solver's own clock
         (SolverOut.time) over the Arnoldi steps and true residuals of those cycles.  The real path is the parent commit's code,
         unchanged.  Operators: a callable of identity cost (an element-wise product with a fixed vector, the same in both halves,
         so that it is complex-linear) at config 2's lengths, 256^2 and 1024^2 (fp64, 2 (3 nx + 1)^2 entries), and the fp32 DDH at
         512^2 (a = 1, omega = 2 pi nx / 10; one cycle).
stall    cd.gmres on the fp32 DDH with a = 1, nx 512, omega = 16 pi, GMRES(20), tol 1e-4, `stall_cycles` cycles, real and complex:
         the residual histories (the real iteration stalls at 0.097 there).
example  matvecs to 1e-4 through the native driver, `ddh_solve nx 4 0.2*nx 20 100 1e-4 - --residuals [--arithmetic complex]`
         (the example's regime and coefficient), nx 256 and 512.

  python profiles/tools/gmres_complex_rates.py [parts=step,example,stall] [cycles=3] [stall_cycles=15]
"""
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import cuddhelmholtz_amd as cd  # noqa: E402

parts = (sys.argv[1] if len(sys.argv) > 1 else "step,example,stall").split(",")
cycles = int(sys.argv[2]) if len(sys.argv) > 2 else 3
stall_cycles = int(sys.argv[3]) if len(sys.argv) > 3 else 15
if not torch.cuda.is_available():
    sys.exit("gmres_complex_rates.py measures on the GPU: none is visible")
dev = torch.device("cuda:0")
cd.use_torch_stream()
M = 20


def step_case(name, n, A, b, n_cycles, reps):
    per = {"real": [], "complex": []}
    for rep in range(reps + 1):  # the first pass warms up
        for arithmetic in ("real", "complex"):
            x = torch.zeros_like(b)
            torch.cuda.synchronize()
            out = cd.gmres(n, x, A, b, M, n_cycles + 1, 0.0, arithmetic=arithmetic)
            assert out.num_iter == n_cycles + 1 and out.num_matvec == 1 + n_cycles * (M + 1), (out.num_iter, out.num_matvec)
            if rep:
                per[arithmetic].append(1e6 * out.time[-1] / (n_cycles * M))
    r, c = np.median(per["real"]), np.median(per["complex"])
    print(f"STEP {name} n={n} GMRES({M}), {n_cycles} cycles x {reps}: real {r:.1f} us per step (min {min(per['real']):.1f}, max {max(per['real']):.1f}), "
          f"complex {c:.1f} us per step (min {min(per['complex']):.1f}, max {max(per['complex']):.1f}), complex / real = {c / r:.3f}", flush=True)


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


if "step" in parts:
    for nx in (256, 1024):
        n = 2 * (3 * nx + 1) ** 2
        g = torch.Generator(device=dev).manual_seed(1)
        half = 1.0 + torch.rand(n // 2, dtype=torch.float64, device=dev, generator=g)
        d = torch.cat([half, half])
        b = torch.randn(n, dtype=torch.float64, device=dev, generator=g)
        step_case(f"identity-cost callable, config 2's {nx}^2, fp64", n, lambda p, q: torch.mul(d, p, out=q), b, cycles, 5 if nx == 256 else 3)  # noqa: B023
        del d, b, half
    F, b, keep = ddh_case(512, 2 * math.pi * 512 / 10)
    step_case("fp32 DDH 512^2", F.size(), F, b, 1, 2)
    print(f"  complex-linearity defect of that operator: {cd.complex_linearity_defect(F, F.size(), 'f32'):.3e}", flush=True)
    del F, b, keep

if "example" in parts:
    exe = ROOT / "build" / "examples" / "ddh_solve"  # (cuddhelmholtz_amd.build.build_examples)
    for nx in (256, 512):
        for extra in ([], ["--arithmetic", "complex"]):
            cmd = [str(exe), str(nx), "4", str(0.2 * nx), "20", "100", "1e-4", "-", "--residuals", *extra]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            print("EXAMPLE $ " + " ".join(["ddh_solve", *cmd[1:]]), flush=True)
            print("  " + "\n  ".join(out.stdout.strip().splitlines()) + (f"\n  exit status {out.returncode}: {out.stderr.strip()}" if out.returncode else ""), flush=True)

if "stall" in parts:
    F, b, keep = ddh_case(512, 16 * math.pi)
    cd.gmres(F.size(), torch.zeros_like(b), F, b, M, 2, 1e-4)  # warm-up: one cycle
    for arithmetic in ("real", "complex"):
        x = torch.zeros_like(b)
        torch.cuda.synchronize()
        out = cd.gmres(F.size(), x, F, b, M, stall_cycles + 1, 1e-4, arithmetic=arithmetic)
        rel = [r / out.res_norm[0] for r in out.res_norm]
        print(f"STALL nx=512 omega=16 pi n={F.size()} GMRES({M}) {arithmetic}: success={out.success} cycles={out.num_iter} matvecs={out.num_matvec} "
              f"seconds={out.time[-1]:.3f} rel_res={rel[-1]:.4e}", flush=True)
        print(f"  residuals {arithmetic}: " + " ".join(f"{r:.4e}" for r in rel), flush=True)
