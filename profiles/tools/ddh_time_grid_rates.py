"""Cost of per-subdomain time grids (DDH(time_step="coefficient")), n_basis 4, fp32, the example's disk coefficient (a = 0.2 for
r < 0.25), BASELINE's omega = pi nx / 32; all plans in one process, timed in alternating rounds.
usage: ddh_time_grid_rates.py [--rounds N] [--reps N] [nx ...]        (default 1024)
  (a) ms per action of the `mesh` plan on kernel 5's matrix form (set_sweep_form(1): the form a plan with time grids takes);
  (b) ms per action of the `coefficient` plan: one launch, the long subdomains first;
  (b') the same launch without the `lambda - update` step (local_traces over the whole range), and
  (c) the `coefficient` plan run as one local_traces_listed call per time grid, one after another.
Reports b / (a * mean ratio), the cost beyond the added time steps, and c / b', what the single sorted launch buys; and, with
a = 1, `coefficient` against `mesh` (the same plan: same form, same time)."""
import math
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import cuddhelmholtz_amd as cd  # noqa: E402

args = sys.argv[1:]
opts = {"--rounds": "3", "--reps": "2"}
while args and args[0] in opts:
    opts[args[0]], args = args[1], args[2:]
rounds, reps = int(opts["--rounds"]), int(opts["--reps"])
dev = torch.device("cuda:0")
cd.use_torch_stream()


def median_ms(v):
    return 1e3 * float(np.median(v))


for nx in (int(v) for v in (args or ["1024"])):
    omega = math.pi * nx / 32.0
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), cd.Basis(4))
    xy = fem.physical_coordinates().reshape(2, -1)
    disk = np.where(xy[0] ** 2 + xy[1] ** 2 < 0.0625, 0.2, 1.0)
    ones = np.ones(fem.size())
    plans = {"mesh": cd.DDH(omega, disk, fem, nx, nx), "coefficient": cd.DDH(omega, disk, fem, nx, nx, time_step="coefficient"),
             "mesh, a = 1": cd.DDH(omega, ones, fem, nx, nx), "coefficient, a = 1": cd.DDH(omega, ones, fem, nx, nx, time_step="coefficient")}
    plans["mesh"].set_sweep_form(1)
    Fc = plans["coefficient"]
    ratios = Fc.time_ratios()
    nd = ratios.size
    lists = [torch.from_numpy(np.flatnonzero(ratios == r).astype(np.int32)).to(dev) for r in sorted(set(ratios), reverse=True)]
    # traces of size 1e-3: the mesh plan's local solves grow by ~1e7 per action inside the disk, the timing must not run on inf / nan
    lam = 1e-3 * torch.rand(Fc.size(), dtype=torch.float32, device=dev)
    out = torch.zeros_like(lam)

    def run(name):
        if name == "traces":
            Fc.local_traces(0, nd, None, lam, out)
        elif name == "listed":
            for ids in lists:
                Fc.local_traces_listed(ids, None, lam, out)
        else:
            plans[name].action(lam, out)

    names = list(plans) + ["traces", "listed"]
    for name in names:  # plans, tables, first launches
        run(name)
    torch.cuda.synchronize()
    times = {name: [] for name in names}
    for _ in range(rounds):
        for name in names:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                run(name)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / reps)
    mean_ratio = float(ratios.mean())
    print(f"nx={nx} subdomains={nd} nt={Fc.info()['nt']} ratios: " + ", ".join(f"{int((ratios == r).sum())} x {int(r)}" for r in sorted(set(ratios)))
          + f"; mean {mean_ratio:.4f}", flush=True)
    for name in names:
        F = plans.get(name, Fc)
        print(f"  {name}: kernel {F.info()['kernel']} form {F.sweep_form()}, ms by round {' '.join(f'{1e3 * v:.2f}' for v in times[name])}; "
              f"median {median_ms(times[name]):.2f}", flush=True)
    a, b, bt, c = (median_ms(times[k]) for k in ("mesh", "coefficient", "traces", "listed"))
    print(f"  b / (a * mean ratio) = {b / (a * mean_ratio):.3f}   (cost beyond the added time steps)")
    print(f"  c / b' = {c / bt:.3f}   (one launch per time grid against the single sorted launch)")
    a1, c1 = median_ms(times["mesh, a = 1"]), median_ms(times["coefficient, a = 1"])
    same = plans["mesh, a = 1"].sweep_form() == plans["coefficient, a = 1"].sweep_form() and plans["coefficient, a = 1"].info()["nt"] == plans["mesh, a = 1"].info()["nt"]
    print(f"  a = 1: coefficient / mesh = {c1 / a1:.3f}, same form and time grid: {same}", flush=True)
    del plans, Fc
