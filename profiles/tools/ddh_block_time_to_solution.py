"""Time to solution by subdomain size and WaveHoltz iterations: rhs -> GMRES(m) on I - T to tol -> postprocess (examples/DDH.cpp:141-144)
for block in {4, 8} x wh_iters in {5, 10, 20}, n_basis 4, fp32 local solves, omega = 2 pi nx / 10 (the example's regime).
usage: ddh_block_time_to_solution.py nx coef(one|disk) m [tol=1e-4] [max_seconds=60]
Per combination: matvecs, seconds of the GMRES call, Krylov memory ((m + 1) vectors of F.size() floats), whether GMRES reached tol
within max_seconds, and the distance of the solution u to that of block 4, wh_iters 20."""
import math
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import cuddhelmholtz_amd as cd  # noqa: E402

nx, coef, m = int(sys.argv[1]), sys.argv[2], int(sys.argv[3])
tol = float(sys.argv[4]) if len(sys.argv) > 4 else 1e-4
max_seconds = float(sys.argv[5]) if len(sys.argv) > 5 else 60.0
omega = 2.0 * math.pi * nx / 10.0
dev = torch.device("cuda:0")
cd.use_torch_stream()
fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), cd.Basis(4))
ndof = fem.size()
f = torch.zeros(2 * ndof, dtype=torch.float64, device=dev)
cd.linear_functional(fem, cd.GAUSSIANS, f[:ndof], param=omega)
a = torch.ones(ndof, dtype=torch.float64, device=dev)
if coef == "disk":  # examples/DDH.cpp:122-125
    cd.linear_functional(fem, cd.ALPHA_DISK, a)
    cd.DiagInvMassMatrix(fem).action(a, a)
h_a = a.cpu().numpy()
print(f"{nx}x{nx}, omega = 2 pi {nx} / 10, coefficient {coef}, GMRES({m}), tol {tol:g}, at most {max_seconds:g} s per solve", flush=True)
rows, ref = [], None
for block, wh in ((4, 20), (4, 10), (4, 5), (8, 20), (8, 10), (8, 5)):
    F = cd.DDH(omega, h_a, fem, nx, nx, block=None if block == 4 else block)
    F.set_wh_iters(wh)
    n = F.size()
    b = torch.zeros(n, dtype=torch.float32, device=dev)
    lam = torch.zeros_like(b)
    F.rhs(f, b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = cd.gmres(n, lam, F, b, m, 100000, tol, verbose=0, max_seconds=max_seconds)
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    u = torch.zeros(2 * ndof, dtype=torch.float64, device=dev)
    F.postprocess(lam, f, u)
    if ref is None:
        ref = u.clone()
    dist = float(torch.linalg.norm(u - ref) / torch.linalg.norm(ref))
    rows.append((block, wh, F.info()["kernel"], n, out.num_matvec, t, 4.0 * (m + 1) * n / 2**20, out.success,
                 out.res_norm[-1] / out.res_norm[0], dist))
    print("block {} wh_iters {:2d} kernel {:2d} traces {:7d}: {:5d} matvecs, {:7.2f} s, Krylov {:7.1f} MiB, reached tol {}, relative residual {:.2e}, "
          "|u - u(block 4, wh 20)| / |u(block 4, wh 20)| = {:.3e}".format(*rows[-1]), flush=True)
    del F
