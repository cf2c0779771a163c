"""Cost per DDH::action by subdomain size: block 4 (auto: kernel 5) against block 8 (auto: kernel 11), n_basis 4, fp32, a = 1,
BASELINE's omega = pi nx / 32, both plans in one process and timed alternately.
usage: ddh_block_rates.py [--rounds N] [--reps N] [--blocks 4,8] nx ...
A library without the block constructor (the commit before; CUDDH_AMD_LIBRARY_VARIANT) is run with --blocks 4."""
import math
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import cuddhelmholtz_amd as cd  # noqa: E402

args = sys.argv[1:]
opts = {"--rounds": "3", "--reps": "3", "--blocks": "4,8"}
while args and args[0] in opts:
    opts[args[0]], args = args[1], args[2:]
rounds, reps, blocks = int(opts["--rounds"]), int(opts["--reps"]), [int(v) for v in opts["--blocks"].split(",")]
dev = torch.device("cuda:0")
cd.use_torch_stream()
for nx in (int(v) for v in args):
    omega = math.pi * nx / 32.0
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), cd.Basis(4))
    plans = {}
    for block in blocks:
        F = cd.DDH(omega, np.ones(fem.size()), fem, nx, nx, block=None if block == 4 else block)
        lam = torch.rand(F.size(), dtype=torch.float32, device=dev)
        out = torch.zeros_like(lam)
        F.action(lam, out)  # plan, tables, first launch
        torch.cuda.synchronize()
        plans[block] = (F, lam, out)
    times = {block: [] for block in blocks}
    for _ in range(rounds):
        for block in blocks:
            F, lam, out = plans[block]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                F.action(lam, out)
            torch.cuda.synchronize()
            times[block].append((time.perf_counter() - t0) / reps)
    for block in blocks:
        F = plans[block][0]
        info = F.info()
        t = times[block]
        print(f"nx={nx} block={block} kernel={info['kernel']} form={F.sweep_form()} subdomains={info['n_domains']} traces={F.size()} nt={info['nt']}: "
              f"ms per action by round {' '.join(f'{1e3 * v:.2f}' for v in t)}; median {1e3 * float(np.median(t)):.2f}, "
              f"{1e9 * float(np.median(t)) / (nx * nx * 5 * info['nt']):.4f} ns per element and time step", flush=True)
    if len(blocks) == 2:
        a, b = (float(np.median(times[k])) for k in blocks)
        print(f"nx={nx}: block {blocks[1]} / block {blocks[0]} = {b / a:.3f}", flush=True)
    del plans
