"""Times DDH::action for several (nx, n_basis, kernel) and prints subdomain RK2 steps per second and the algorithmic
fp32 FLOP rate (2*nb*2 + 6 + 2*nb*2 + 1 per node per sweep, 26 per node per step for the update).
usage: ddh_rates.py [--reps N] "nx[xny],nb,kernel[,form[,order[,forcing]]]" ...      nx, ny: elements per side; form: kernel 5's sweep form (DDH.set_sweep_form: 1 matrix, 2 element-lane);
order: the element-lane form's chain order (DDH.set_chain_order: 1 pinned, 2 paired); forcing: where its march applies the sources
(DDH.set_forcing: 1 every WaveHoltz pass, 2 the first only)"""
import math
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import cuddhelmholtz_amd as cd  # noqa: E402

dev = torch.device("cuda:0")
cd.use_torch_stream()
specs = sys.argv[1:]
reps = 3
if specs[:1] == ["--reps"]:
    reps, specs = int(specs[1]), specs[2:]
for spec in specs:
    size, *rest = spec.split(",")
    nx, ny = (int(v) for v in (size.split("x") * 2)[:2])
    nb, kernel, form, order, forcing = (*(int(v) for v in rest), 0, 0, 0)[:5]
    omega = math.pi * nx / 32.0
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, ny, -1.0, 1.0), cd.Basis(nb))
    F = cd.DDH(omega, np.ones(fem.size()), fem, nx, ny, kernel=kernel)
    if form:
        F.set_sweep_form(form)
    if order:
        F.set_chain_order(order)
    if forcing:
        F.set_forcing(forcing)
    info = F.info()
    lam = torch.rand(F.size(), dtype=torch.float32, device=dev)
    out = torch.zeros_like(lam)
    F.action(lam, out)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        F.action(lam, out)
    torch.cuda.synchronize()
    t = (time.perf_counter() - t0) / reps
    nodes = (nb * info["nel1d"]) ** 2
    steps = 5 * info["nt"] * info["n_domains"]
    flops = steps * nodes * (2 * (8 * nb + 7) + 26)
    print(f"nx={nx} ny={ny} nb={nb} kernel={info['kernel']} form={F.sweep_form()} order={F.chain_order()} forcing={F.forcing()} subdomains={info['n_domains']} nodes/subdomain={nodes} nt={info['nt']}: "
          f"{t * 1e3:.1f} ms per action, {steps / t / 1e9:.3f} G subdomain-steps/s, {flops / t / 1e12:.1f} TFLOP/s "
          f"({100 * flops / t / 157.3e12:.0f} % of fp32 vector peak), {2 * fem.size() / t / 1e6:.1f} M DoF*iter/s")
    del F, fem
