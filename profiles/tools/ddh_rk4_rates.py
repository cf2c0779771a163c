"""Cost of DDH.action with RK4 local solves on a coarser grid against RK2 on the mesh grid: n_basis 4, fp32, kernel 5 in the matrix
form (the form an RK4 plan takes), a == 1, BASELINE's omega = pi nx / 32; all plans in one process, timed in alternating rounds.
usage: ddh_rk4_rates.py [--rounds N] [--reps N] [--out FILE] [nx ...]        (default 512 1024; FILE default
       profiles/r13/ddh_rk4_rates.txt, relative to the repository)
Per nx: ms per action of  rk2 (nt_mesh steps, 2 sweeps each),  rk4 at coarsen 4 and 8 (ceil(nt_mesh / c) steps, 4 sweeps each),
and rk4 at coarsen 1 (the cost of a step alone); beside each the sweeps per local solve, 2 or 4 x nt x wh_iters, and the time per
sweep in ns (the action's time over the sweeps of one subdomain: all subdomains march in one launch).  Then the ratio to rk2
against the coarsen / 2 that the sweep count predicts.  A spread line repeats rk2 against itself (first half of its rounds against
the second): differences below it mean nothing."""
import math
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import cuddhelmholtz_amd as cd  # noqa: E402

args = sys.argv[1:]
opts = {"--rounds": "6", "--reps": "2", "--out": str(ROOT / "profiles" / "r13" / "ddh_rk4_rates.txt")}
while args and args[0] in opts:
    opts[args[0]], args = args[1], args[2:]
rounds, reps = int(opts["--rounds"]), int(opts["--reps"])
if not torch.cuda.is_available():
    sys.exit("ddh_rk4_rates.py: no GPU; a time is measured on the device or not at all")
dev = torch.device("cuda:0")
cd.use_torch_stream()
WH_ITERS = 5
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


say(f"ddh_rk4_rates.py --rounds {rounds} --reps {reps}: {torch.cuda.get_device_name(0)}; ms per DDH.action, median over rounds")
for nx in (int(v) for v in (args or ["512", "1024"])):
    omega = math.pi * nx / 32.0
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), cd.Basis(4))
    ones = np.ones(fem.size())
    plans = {"rk2": cd.DDH(omega, ones, fem, nx, nx, kernel=5)}
    plans["rk2"].set_sweep_form(1)
    for c in (4, 8, 1):
        plans[f"rk4 / {c}"] = cd.DDH(omega, ones, fem, nx, nx, kernel=5, integrator="rk4", coarsen=c)
    lam = torch.rand(plans["rk2"].size(), dtype=torch.float32, device=dev)
    out = torch.zeros_like(lam)
    names = list(plans)
    for name in names:  # plans, tables, first launches
        plans[name].action(lam, out)
    torch.cuda.synchronize()
    times = {name: [] for name in names}
    for _ in range(rounds):
        for name in names:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                plans[name].action(lam, out)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / reps)
    info = plans["rk2"].info()
    say(f"nx={nx} subdomains={info['n_domains']} nt_mesh={info['nt']} wh_iters={WH_ITERS}")
    med = {}
    for name in names:
        F = plans[name]
        scheme, c = F.integrator()
        sweeps = (4 if scheme == "rk4" else 2) * F.info()["nt"] * WH_ITERS
        med[name] = 1e3 * float(np.median(times[name]))
        say(f"  {name}: kernel {F.info()['kernel']} form {F.sweep_form()}, nt {F.info()['nt']}, {sweeps} sweeps per local solve; ms by round "
            f"{' '.join(f'{1e3 * v:.2f}' for v in times[name])}; median {med[name]:.2f} ms, {1e6 * med[name] / sweeps:.1f} ns per sweep")
    half = rounds // 2
    if half:
        a, b = np.median(times["rk2"][:half]), np.median(times["rk2"][half:])
        say(f"  spread: rk2, first {half} rounds against the rest: {abs(a - b) / min(a, b) * 100:.2f} %")
    for c in (4, 8):
        say(f"  rk2 / (rk4 / {c}) = {med['rk2'] / med[f'rk4 / {c}']:.3f}   (the sweep count predicts {c / 2:.1f})")
    say(f"  (rk4 / 1) / rk2 = {med['rk4 / 1'] / med['rk2']:.3f}   (an RK4 step against an RK2 step; the sweep count predicts 2.0)")
    del plans
out_path = Path(opts["--out"])
out_path.parent.mkdir(parents=True, exist_ok=True)
out_path.write_text("\n".join(lines) + "\n")
