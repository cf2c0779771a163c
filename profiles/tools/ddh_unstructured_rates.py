"""DDH local solves on config 5's unstructured mesh: times DDH::action of a label-built DDH (DDH.from_labels) with kernel 9
(one wavefront per subdomain, LDS assembly along CSR lists) and kernel 10 (one workgroup per subdomain) in the SAME process,
fp32 and fp64, a = 1, one warm-up action, best and mean of `reps`.

mesh: Mesh2D.load(tests/golden/unstructured_square).refined(5) (121,856 quads), n_basis 4, partition(ceil(n_elem / 16)) so
that every part has <= 16 elements; omega = pi * nx_eq / 32 with nx_eq = sqrt(n_elem) (BASELINE's 32 elements per wavelength
on a uniform mesh of as many elements).  For context the block kernels 3 and 5 (fp32) / 3 and 8 (fp64) run on a uniform_rect
with about as many 4x4-element subdomains at the same omega.

Prints ms per action, M DoF*iter/s (2 * ndof per action, bench.py's unit), G subdomain-steps/s and the executed FLOP rate as a
fraction of the 157.3 TF fp32 / 78.6 TF fp64 peak, counted per element node per RK2 step as
  kernels 3, 9, 10: 2 sweeps x (8 nb + 7 + 1) + 26 (update) = 106 at nb 4  (ddh_rates.py's 104 + one assembly add per node
                    and sweep; the kernels 3 / 5 / 8 rows use it too, so that the rows compare time for the same work)
usage: ddh_unstructured_rates.py [--refine R] [--reps N] [--k10-domains M]
  --k10-domains M: time kernel 10 on M listed subdomains (local_traces_listed) and scale, instead of whole actions"""
import argparse
import math
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import cuddhelmholtz_amd as cd  # noqa: E402

PEAK = {"f32": 157.3e12, "f64": 78.6e12}
FLOP_PER_NODE_STEP = 2 * (8 * 4 + 7 + 1) + 26

ap = argparse.ArgumentParser()
ap.add_argument("--refine", type=int, default=5)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--k10-domains", type=int, default=0)
args = ap.parse_args()

dev = torch.device("cuda:0")
cd.use_torch_stream()


def timed(fn, reps):
    fn()  # warm-up (plan, code object load)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts), sum(ts) / len(ts)


def report(tag, prec, F, fem, t, mean, n_dom_timed=None):
    info = F.info()
    nd = info["n_domains"] if n_dom_timed is None else n_dom_timed
    steps = 5 * info["nt"] * nd
    nodes = 256
    flops = steps * nodes * FLOP_PER_NODE_STEP
    scale = info["n_domains"] / nd  # listed subsets: per-action time scaled to all subdomains
    print(f"{tag} {prec} kernel={info['kernel']} subdomains={info['n_domains']} nt={info['nt']}"
          + (f" (timed on {nd} listed)" if n_dom_timed else "")
          + f": {t * scale * 1e3:.1f} ms per action (mean {mean * scale * 1e3:.1f}), {2 * fem.size() / (t * scale) / 1e6:.2f} M DoF*iter/s, "
          f"{steps / t / 1e9:.3f} G subdomain-steps/s, {flops / t / 1e12:.1f} TFLOP/s = {100 * flops / t / PEAK[prec]:.0f} % of the "
          f"{prec} peak", flush=True)
    return t * scale


mesh = cd.Mesh2D.load(ROOT / "tests" / "golden" / "unstructured_square").refined(args.refine)
n_elem = mesh.n_elem()
labels = mesh.partition(math.ceil(n_elem / 16))
nx_eq = math.sqrt(n_elem)
omega = math.pi * nx_eq / 32.0
fem = cd.H1Space(mesh, cd.Basis(4))
print(f"mesh: unstructured_square refined {args.refine}x = {n_elem} quads, {labels.max() + 1} parts of <= {np.bincount(labels).max()} "
      f"elements, ndof {fem.size()}, omega {omega:.3f}", flush=True)
nxu = 4 * max(1, round(nx_eq / 4))
# element side 1/128 exactly: every element of the uniform mesh has bitwise the same metric, which kernels 5 and 8 require
fem_u = cd.H1Space(cd.Mesh2D.uniform_rect(nxu, 0.0, nxu / 128.0, nxu, 0.0, nxu / 128.0), cd.Basis(4))

for prec in ("f32", "f64"):
    dt = torch.float32 if prec == "f32" else torch.float64
    times = {}
    for kernel in (9, 10):
        F = cd.DDH.from_labels(omega, np.ones(fem.size()), fem, labels, precision=prec, kernel=kernel)
        assert F.info()["kernel"] == kernel
        lam = torch.rand(F.size(), dtype=dt, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        out = torch.zeros_like(lam)
        if kernel == 10 and args.k10_domains:
            ids = torch.arange(args.k10_domains, dtype=torch.int32, device=dev)
            t, mean = timed(lambda: F.local_traces_listed(ids, None, lam, out), args.reps)
            times[kernel] = report("unstructured", prec, F, fem, t, mean, args.k10_domains)
        else:
            t, mean = timed(lambda: F.action(lam, out), args.reps)
            times[kernel] = report("unstructured", prec, F, fem, t, mean)
        del F, lam, out
    print(f"unstructured {prec}: kernel 9 / kernel 10 speed-up {times[10] / times[9]:.2f}x", flush=True)
    for kernel in ((3, 5) if prec == "f32" else (3, 8)):
        F = cd.DDH(omega, np.ones(fem_u.size()), fem_u, nxu, nxu, precision=prec, kernel=kernel)
        lam = torch.rand(F.size(), dtype=dt, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        out = torch.zeros_like(lam)
        t, mean = timed(lambda: F.action(lam, out), args.reps)
        report(f"uniform_rect {nxu}^2", prec, F, fem_u, t, mean)
        del F, lam, out
