"""fp64 DDH local solves: times DDH64::action with kernel 2 (sum-factorised, VALU) and kernel 8 (dense element matrix on
v_mfma_f64_16x16x4_f64) in the SAME process, a = 1, omega = pi nx / 32 (BASELINE's 32 elements per wavelength), float64 traces,
one warm-up action, best and mean of `reps`.  Prints ms per action, M DoF*iter/s (2 * ndof per action, bench.py's unit), and
the executed FLOP rate as a fraction of the 78.6 TF fp64 peak, counted per node per RK2 step as
  kernel 2: 2 sweeps x (8 nb + 7) + 26 (update)       = 104 at nb 4   (ddh_rates.py's count)
  kernel 8: 2 sweeps x (2 x 16 + 3) + 26 (update)     =  96           (one 16-term dot per output node + assembly)
usage: ddh64_rates.py [nx ...] [--reps R]   (default: 512 1024, R = 3)"""
import argparse
import math
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import cuddhelmholtz_amd as cd  # noqa: E402

PEAK_F64 = 78.6e12
FLOP_PER_NODE_STEP = {2: 2 * (8 * 4 + 7) + 26, 8: 2 * (2 * 16 + 3) + 26}

ap = argparse.ArgumentParser()
ap.add_argument("nx", type=int, nargs="*", default=[512, 1024])
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()

dev = torch.device("cuda:0")
cd.use_torch_stream()
for nx in args.nx:
    omega = math.pi * nx / 32.0
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), cd.Basis(4))
    rates = {}
    for kernel in (2, 8):
        F = cd.DDH(omega, np.ones(fem.size()), fem, nx, nx, precision="f64", kernel=kernel)
        info = F.info()
        assert info["kernel"] == kernel, info
        lam = torch.rand(F.size(), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        out = torch.zeros_like(lam)
        F.action(lam, out)  # warm-up (plan, code object load)
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            F.action(lam, out)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        t = min(ts)
        nodes = 256
        steps = 5 * info["nt"] * info["n_domains"]
        flops = steps * nodes * FLOP_PER_NODE_STEP[kernel]
        rates[kernel] = t
        print(f"nx={nx} f64 kernel={kernel} subdomains={info['n_domains']} nt={info['nt']}: {t * 1e3:.1f} ms per action "
              f"(mean {1e3 * sum(ts) / len(ts):.1f}), {2 * fem.size() / t / 1e6:.2f} M DoF*iter/s, {flops / t / 1e12:.1f} TFLOP/s "
              f"= {100 * flops / t / PEAK_F64:.0f} % of the fp64 peak, {steps / t / 1e9:.3f} G subdomain-steps/s", flush=True)
        del F, lam, out
    print(f"nx={nx}: kernel 8 / kernel 2 speed-up {rates[2] / rates[8]:.2f}x", flush=True)
