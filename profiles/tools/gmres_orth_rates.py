"""us per matvec of GMRES under orth="mgs" and orth="cgs2" in the same run, alternating (method of profiles/tools/gmres_helm.py:
wall time of the solve between device synchronisations, tol so small that every cycle runs, a warm-up solve per variant first).

  config 2's shape   HelmholtzOperator::gmres (plan-native vectors), 256^2, n_basis 4, omega = 8 pi, GMRES(20)
  the same at 1024^2 (omega = 32 pi as gmres_helm.py scales it)
  fp32 DDH           cd.gmres on the DDH operator, 512^2, n_basis 4, omega = 16 pi, GMRES(20)

One line per (case, orth, repeat) and a summary line per case with the median of each and their ratio.  Needs one MI355X.
  python profiles/tools/gmres_orth_rates.py [cycles=10] [repeats=3] [cases=helm256,helm1024,ddh512]
"""
import math
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import cuddhelmholtz_amd as cd  # noqa: E402

cycles = int(sys.argv[1]) if len(sys.argv) > 1 else 10
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
cases = (sys.argv[3] if len(sys.argv) > 3 else "helm256,helm1024,ddh512").split(",")
if not torch.cuda.is_available():
    sys.exit("gmres_orth_rates.py measures on the GPU: none is visible")
dev = torch.device("cuda:0")
cd.use_torch_stream()


def helmholtz(nx):
    omega = math.pi * nx / 32.0
    mesh = cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0)
    fem = cd.H1Space(mesh, cd.Basis(4))
    n = fem.size()
    fs = cd.FaceSpace(fem, mesh.boundary_edges())
    a2 = torch.zeros(n, dtype=torch.float64, device=dev)
    cd.nodal_values(fem, cd.ALPHA_DISK_SQ, a2)
    A = cd.HelmholtzOperator(omega, a2, torch.ones(fs.size(), dtype=torch.float64, device=dev), fem, fs)
    b = torch.zeros(2 * n, dtype=torch.float64, device=dev)
    cd.linear_functional(fem, cd.GAUSSIANS, b[:n], param=omega)
    x = torch.zeros_like(b)
    return f"helmholtz nx={nx} N={2 * n} native={A.has_native()} kernel {A.kernel()}", x, (lambda orth: A.gmres(x, b, 20, cycles + 1, 1e-30, orth=orth)), (mesh, fem, fs, A)


def ddh(nx):
    omega = math.pi * nx / 32.0
    mesh = cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0)
    fem = cd.H1Space(mesh, cd.Basis(4))
    n = fem.size()
    F = cd.DDH(omega, torch.ones(n, dtype=torch.float64).numpy(), fem, nx, nx)
    f = torch.zeros(2 * n, dtype=torch.float64, device=dev)
    cd.linear_functional(fem, cd.GAUSSIANS, f[:n], param=omega)
    b = torch.zeros(F.size(), dtype=torch.float32, device=dev)
    F.rhs(f, b)
    x = torch.zeros_like(b)
    return f"ddh fp32 nx={nx} n_lambda={F.size()} kernel {F.info()['kernel']}", x, (lambda orth: cd.gmres(F.size(), x, F, b, 20, cycles + 1, 1e-30, orth=orth)), (mesh, fem, F)


BUILD = {"helm256": lambda: helmholtz(256), "helm1024": lambda: helmholtz(1024), "ddh512": lambda: ddh(512)}

for case in cases:
    name, x, solve, keep = BUILD[case]()
    rates = {"mgs": [], "cgs2": []}
    for rep in range(repeats + 1):  # the first pass warms up
        for orth in ("mgs", "cgs2"):
            x.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = solve(orth)
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            if rep:
                rates[orth].append(1e6 * t / out.num_matvec)
                print(f"{name} orth={orth} rep={rep}: matvecs={out.num_matvec} seconds={t:.4f} us_per_matvec={1e6 * t / out.num_matvec:.1f} "
                      f"rel_res={out.res_norm[-1] / out.res_norm[0]:.3e}", flush=True)
    m, c = statistics.median(rates["mgs"]), statistics.median(rates["cgs2"])
    print(f"SUMMARY {name} GMRES(20) x {cycles} cycles: mgs {m:.1f} us/matvec (min {min(rates['mgs']):.1f}, max {max(rates['mgs']):.1f}), "
          f"cgs2 {c:.1f} us/matvec (min {min(rates['cgs2']):.1f}, max {max(rates['cgs2']):.1f}), cgs2 / mgs = {c / m:.3f}", flush=True)
    del keep, solve
