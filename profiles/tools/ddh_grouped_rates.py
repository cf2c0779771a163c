"""Cost per DDH::action of kernel 13 (the element-lane local solves with four subdomains per wavefront on per-subdomain time
grids) against what the same plan runs without it, fp32, block 4: all plans of one case from one build on the same inputs in
one process, alternating, timed with device events (the method of ddh_nb5_rates.py).
usage: ddh_grouped_rates.py [--rounds N] [--reps N] [--limit SECONDS] [--sizes4 NX,..] [--sizes5 NX,..]     every case, a child process each
       ddh_grouped_rates.py [--rounds N] [--reps N] --case NB NX COEF                                       one case in this process
Cases: n_basis 5 at nx = 32, 128, 512 (64, 1,024, 16,384 subdomains) and n_basis 4 at nx = 128, 512 (1,024, 16,384; 1024 for
65,536 through --sizes4), omega = 2 pi nx / 10 (nt 1250 / 800 on the mesh grid), each with
  COEF disk: the examples' disk coefficient (a = 0.2 for r < 0.25) under time_step="coefficient" (ratios 1 and 5):
             kernel 13 against today's kernel for such a plan (n_basis 5: kernel 1; n_basis 4: kernel 5, matrix form);
  COEF ones: a = 1 with an explicit all-ones ratio array (the instantiations with time grids, one pass per wavefront): the same
             two, and the one-grid element-lane kernel on time_step="mesh" (kernel 12; kernel 5 with set_sweep_form(2)), which
             gives the cost of the grid lookup and the pass loop.
Every case runs as a child process under its own time limit; the first that fails ends the run."""
import math
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
args = sys.argv[1:]
opts = {"--rounds": "3", "--reps": "2", "--limit": "300", "--sizes4": "128,512", "--sizes5": "32,128,512"}
while args and args[0] in opts:
    opts[args[0]], args = args[1], args[2:]
rounds, reps = int(opts["--rounds"]), int(opts["--reps"])

if not args:
    sizes = [(5, int(v)) for v in opts["--sizes5"].split(",") if v] + [(4, int(v)) for v in opts["--sizes4"].split(",") if v]
    for nb, nx in sizes:
        for coef in ("disk", "ones"):
            r = subprocess.run([sys.executable, __file__, "--rounds", str(rounds), "--reps", str(reps), "--case", str(nb), str(nx), coef],
                               timeout=float(opts["--limit"]))
            if r.returncode != 0:
                sys.exit(f"n_basis {nb} nx={nx} {coef}: exit status {r.returncode}; stopping")
    sys.exit(0)

assert args[0] == "--case" and len(args) == 4 and args[3] in ("disk", "ones"), __doc__
import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, str(ROOT))
import cuddhelmholtz_amd as cd  # noqa: E402

nb, nx, coef = int(args[1]), int(args[2]), args[3]
omega = 2.0 * math.pi * nx / 10.0
dev = torch.device("cuda:0")
cd.use_torch_stream()
fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), cd.Basis(nb))
nd = (nx // 4) ** 2
if coef == "disk":
    xy = fem.physical_coordinates().reshape(2, -1)
    h_a, time_step = np.where(xy[0] ** 2 + xy[1] ** 2 < 0.0625, 0.2, 1.0), "coefficient"
else:
    h_a, time_step = np.ones(fem.size()), np.ones(nd, dtype=np.int32)
today = 1 if nb == 5 else 5
# name: (kernel, time_step, sweep form to set)
specs = {"kernel 13": (13, time_step, None), f"kernel {today}": (today, time_step, None)}
if coef == "ones":
    specs["one grid, element-lane"] = (12, "mesh", None) if nb == 5 else (5, "mesh", 2)
plans = {}
for name, (k, ts, form) in specs.items():
    F = cd.DDH(omega, h_a, fem, nx, nx, kernel=k, block=4, time_step=ts)
    if form is not None:
        F.set_sweep_form(form)
    lam = 1e-3 * torch.rand(F.size(), dtype=torch.float32, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    out = torch.zeros_like(lam)
    F.action(lam, out)  # plan, tables, first launch
    torch.cuda.synchronize()
    assert F.info()["kernel"] == k and F.info()["n_domains"] == nd
    plans[name] = (F, lam, out)
ratios = plans["kernel 13"][0].time_ratios()
assert list(ratios) == list(plans[f"kernel {today}"][0].time_ratios())
ref = plans[f"kernel {today}"][2]
times = {name: [] for name in plans}
for _ in range(rounds):
    for name, (F, lam, out) in plans.items():
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(reps):
            F.action(lam, out)
        stop.record()
        torch.cuda.synchronize()
        times[name].append(start.elapsed_time(stop) / reps)  # ms
info = plans["kernel 13"][0].info()
head = f"nb={nb} block=4 nx={nx} {coef} subdomains={nd} nt={info['nt']}"
print(f"{head}: ratios " + ", ".join(f"{int((ratios == r).sum())} x {int(r)}" for r in sorted(set(ratios))) + f"; mean {float(ratios.mean()):.4f}", flush=True)
for name, (F, lam, out) in plans.items():
    t = times[name]
    print(f"{head} {name} (sweep form {F.sweep_form()}, time grids: {'yes' if name != 'one grid, element-lane' else 'no'}): ms per action by round "
          f"{' '.join(f'{v:.3f}' for v in t)}; median {float(np.median(t)):.3f}; action against kernel {today}, relative 2-norm "
          f"{float((out - ref).norm() / ref.norm()):.2e}", flush=True)
med = {name: float(np.median(t)) for name, t in times.items()}
by_round = [a / b for a, b in zip(times[f"kernel {today}"], times["kernel 13"])]
print(f"{head}: kernel {today} / kernel 13 by round {' '.join(f'{v:.3f}' for v in by_round)}; of the medians {med[f'kernel {today}'] / med['kernel 13']:.3f}", flush=True)
if coef == "ones":
    by_round = [a / b for a, b in zip(times["kernel 13"], times["one grid, element-lane"])]
    print(f"{head}: kernel 13 with time grids / one-grid element-lane kernel by round {' '.join(f'{v:.3f}' for v in by_round)}; of the medians "
          f"{med['kernel 13'] / med['one grid, element-lane']:.3f}", flush=True)
