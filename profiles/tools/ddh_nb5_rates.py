"""Cost per DDH::action at n_basis 5, block 4, fp32, a = 1: kernel 12 (ddh_element_lane_kernel<5, ..>) against kernel 1
(ddh_block_kernel) of the same build on the same plan inputs, in one process, alternating, timed with device events.
usage: ddh_nb5_rates.py [--rounds N] [--reps N] [--limit SECONDS]            every size below, one child process each
       ddh_nb5_rates.py [--rounds N] [--reps N] --case NX OMEGA_OVER_PI      one size in this process
Sizes: nx = 32, 64, 128, 256, 512 elements per side (64 ... 16,384 subdomains) at omega = 2 pi nx / 10 (nt 1250), and 512 at
BASELINE's omega = 16 pi (nt 8000).  Every size runs as a child process under its own time limit; the first that fails
ends the run."""
import math
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
args = sys.argv[1:]
opts = {"--rounds": "3", "--reps": "2", "--limit": "420"}
while args and args[0] in opts:
    opts[args[0]], args = args[1], args[2:]
rounds, reps = int(opts["--rounds"]), int(opts["--reps"])

if not args:
    cases = [(nx, 2.0 * nx / 10.0) for nx in (32, 64, 128, 256, 512)] + [(512, 16.0)]
    for nx, w in cases:
        r = subprocess.run([sys.executable, __file__, "--rounds", str(rounds), "--reps", str(reps), "--case", str(nx), repr(w)],
                           timeout=float(opts["--limit"]))
        if r.returncode != 0:
            sys.exit(f"nx={nx} omega={w} pi: exit status {r.returncode}; stopping")
    sys.exit(0)

assert args[0] == "--case" and len(args) == 3, __doc__
import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, str(ROOT))
import cuddhelmholtz_amd as cd  # noqa: E402

nx, omega = int(args[1]), math.pi * float(args[2])
dev = torch.device("cuda:0")
cd.use_torch_stream()
fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), cd.Basis(5))
kernels = (12, 1)
plans = {}
for k in kernels:
    F = cd.DDH(omega, np.ones(fem.size()), fem, nx, nx, kernel=k, block=4)
    lam = torch.rand(F.size(), dtype=torch.float32, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    out = torch.zeros_like(lam)
    F.action(lam, out)  # plan, tables, first launch
    torch.cuda.synchronize()
    assert F.info()["kernel"] == k
    plans[k] = (F, lam, out)
d = float((plans[12][2] - plans[1][2]).norm() / plans[1][2].norm())
times = {k: [] for k in kernels}
for _ in range(rounds):
    for k in kernels:
        F, lam, out = plans[k]
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(reps):
            F.action(lam, out)
        stop.record()
        torch.cuda.synchronize()
        times[k].append(start.elapsed_time(stop) / reps)  # ms
info = plans[12][0].info()
head = f"nx={nx} nb=5 block=4 omega={float(args[2]):g} pi subdomains={info['n_domains']} nt={info['nt']}"
for k in kernels:
    t = times[k]
    med = float(np.median(t))
    print(f"{head} kernel={k}: ms per action by round {' '.join(f'{v:.3f}' for v in t)}; median {med:.3f}, "
          f"{2 * fem.size() / (1e-3 * med) / 1e6:.2f} M DoF*iter/s", flush=True)
r = [a / b for a, b in zip(times[1], times[12])]
print(f"{head}: kernel 1 / kernel 12 by round {' '.join(f'{v:.3f}' for v in r)}; of the medians "
      f"{float(np.median(times[1])) / float(np.median(times[12])):.3f}; action of 12 against 1, relative 2-norm {d:.2e}", flush=True)
