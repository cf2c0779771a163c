"""What the three-dimensional box sweeps cost on one MI355X, n_basis 4, a == 1, homogeneous form.

step     per size (n^3 elements): us per sweep of cuddh_hip_wave_box_* averaged over an RK2 step (rk2_a, rk2_b) and over an RK4 step
         (rk4_1 .. rk4_4, with the march's ps ping-pong), and TB/s on the stated bytes (18 / 46 vectors of 8 B per slot and step,
         as in two dimensions), beside two things measured in the same run, alternating, device events around `inner` back-to-back
         steps, medians of `reps`:
           (a) the stage alone, cuddh_hip_wave_stage_*, on vectors of the same length: the floor the bytes set (it reads w instead
               of computing it: 19 / 47 vectors per step);
           (b) the 2-D lattice sweeps, cuddh_hip_wave_lattice_*, at the nearest node count, compared per node.
period   ms per homogeneous period of cd.WaveHoltzBox, rk2 and rk4 / 4, omega = 2 pi n / 10 on [-1, 1]^3.
solve    one whole solve: omega = 2 pi n / 10, a == 1, one Gaussian load, rk4 / 4, GMRES(20), tol 1e-4: matvecs and seconds.

  python profiles/tools/waveholtz_box_rates.py [parts=step,period,solve] [sizes=32,64,128] [period_sizes=32,64] [solve_sizes=64] [reps=7] [out=profiles/r34/wave_box_rates.txt]
"""
import ctypes as C
import math
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import cuddhelmholtz_amd as cd  # noqa: E402
from cuddhelmholtz_amd import _native as N  # noqa: E402

argv = dict(a.split("=", 1) for a in sys.argv[1:])
parts = argv.get("parts", "step,period,solve").split(",")
sizes = [int(v) for v in argv.get("sizes", "32,64,128").split(",") if v]
period_sizes = [int(v) for v in argv.get("period_sizes", "32,64").split(",") if v]
solve_sizes = [int(v) for v in argv.get("solve_sizes", "64").split(",") if v]
reps = int(argv.get("reps", "7"))
out_path = Path(argv.get("out", str(ROOT / "profiles" / "r34" / "wave_box_rates.txt")))
if not torch.cuda.is_available():
    sys.exit("waveholtz_box_rates.py measures on the GPU: none is visible")
dev = torch.device("cuda:0")
cd.use_torch_stream()
NB = 4
NEAREST_2D = {32: 318, 64: 1024, 128: 2518}  # nx of the 2-D lattice whose node count is nearest (64: the size DESIGN 4.5.1 records)
VECTORS = {"rk2": 18, "rk4": 46}
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text("\n".join(lines) + "\n")


def p(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def timed(fs, inner):
    """median ms per call of every f in fs (name -> callable), alternating, `reps` passes after two warm-up passes"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = {k: [] for k in fs}
    for rep in range(reps + 2):
        for k, f in fs.items():
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(inner):
                f()
            ev[1].record()
            torch.cuda.synchronize()
            if rep >= 2:
                times[k].append(ev[0].elapsed_time(ev[1]) / inner)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def vectors(m, Lx, stride):
    g = torch.Generator(device=dev).manual_seed(1)
    v = {k: torch.randn(m, dtype=torch.float64, device=dev, generator=g) for k in ("w", "p", "q", "u", "v", "ps", "ps2", "qs", "aq", "ap")}
    v["invm"] = torch.rand(m, dtype=torch.float64, device=dev, generator=g) + 0.5
    v["Hi"] = torch.zeros(m, dtype=torch.float64, device=dev)
    if stride > Lx:  # the padding columns: zero state, invm = 0
        for t in v.values():
            t.view(-1, stride)[:, Lx:] = 0.0
    return v


def steps(fn, d, a, st):
    """(rk2 step, rk4 step) of the one-sweep entry points fn(name), with the march's buffers"""
    dt = 1e-9  # (the timed launches repeat on the same vectors: keep them bounded)

    def rk2():
        N.check(fn("rk2_a")(d, dt / 2, 1.0, 0.0, a["p"], a["q"], a["invm"], a["Hi"], None, None, a["qs"], a["ps"], st))
        N.check(fn("rk2_b")(d, dt, 1.0, 0.0, 1e-3, a["ps"], a["qs"], a["invm"], a["Hi"], None, None, a["p"], a["q"], a["u"], a["v"], st))

    def rk4():
        N.check(fn("rk4_1")(d, dt / 2, 1.0, 0.0, a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps"], a["qs"], a["aq"], a["ap"], st))
        N.check(fn("rk4_2")(d, dt / 2, 1.0, 0.0, a["ps"], a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps2"], a["qs"], a["aq"], a["ap"], st))
        N.check(fn("rk4_3")(d, dt, 1.0, 0.0, a["ps2"], a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps"], a["qs"], a["aq"], a["ap"], st))
        N.check(fn("rk4_4")(d, dt / 6, 1.0, 0.0, 1e-3, a["ps"], a["qs"], a["aq"], a["ap"], a["invm"], a["Hi"], None, None, a["p"], a["q"], a["u"], a["v"], st))

    return rk2, rk4


def stage_steps(n, a, st):
    """the stages alone on n elements: w is read, not computed"""
    L, dt = N.lib, 1e-9

    def rk2():
        N.check(L.cuddh_hip_wave_stage_rk2_a_f64(n, dt / 2, 1.0, 0.0, a["w"], a["p"], a["q"], a["invm"], a["Hi"], None, None, a["qs"], a["ps"], st))
        N.check(L.cuddh_hip_wave_stage_rk2_b_f64(n, dt, 1.0, 0.0, 1e-3, a["w"], a["qs"], a["invm"], a["Hi"], None, None, a["p"], a["q"], a["u"], a["v"], st))

    def rk4():
        N.check(L.cuddh_hip_wave_stage_rk4_1_f64(n, dt / 2, 1.0, 0.0, a["w"], a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps"], a["qs"], a["aq"], a["ap"], st))
        N.check(L.cuddh_hip_wave_stage_rk4_2_f64(n, dt / 2, 1.0, 0.0, a["w"], a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps"], a["qs"], a["aq"], a["ap"], st))
        N.check(L.cuddh_hip_wave_stage_rk4_3_f64(n, dt, 1.0, 0.0, a["w"], a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps"], a["qs"], a["aq"], a["ap"], st))
        N.check(L.cuddh_hip_wave_stage_rk4_4_f64(n, dt / 6, 1.0, 0.0, 1e-3, a["w"], a["qs"], a["aq"], a["ap"], a["invm"], a["Hi"], None, None, a["p"], a["q"], a["u"], a["v"], st))

    return rk2, rk4


def box_description(n):
    D, unit = N.WaveBox(), np.array([-1.0, 1.0] * 3)
    N.check_capi(N.lib.cuddh_wave_box_describe(n, n, n, unit.ctypes.data, NB, None, 63, C.byref(D), None, None, None, None, None, None, None))
    return D


def lattice_description(nx):
    Lx = nx * (NB - 1) + 1
    D = N.WaveLattice()
    D.nx, D.ny, D.n_basis, D.stride, D.cx, D.cy = nx, nx, NB, Lx + Lx % 2, 1.0, 1.0
    A, w, basis = np.zeros((NB, NB)), np.zeros(NB), cd.Basis(NB)
    N.check_capi(N.lib.cuddh_wave_lattice_tables(basis._h, A.ctypes.data, w.ctypes.data))
    for i, x in enumerate(A.reshape(-1)):
        D.A[i] = x
    for i, x in enumerate(w):
        D.w[i] = x
    return D, Lx


def step(n):
    L, st = N.lib, stream()
    D3 = box_description(n)
    L3 = n * (NB - 1) + 1
    m3 = D3.stride * L3 * L3
    v3 = vectors(m3, L3, D3.stride)
    a3 = {k: p(t) for k, t in v3.items()}
    box2, box4 = steps(lambda name: getattr(L, f"cuddh_hip_wave_box_{name}_f64"), C.byref(D3), a3, st)
    stage2, stage4 = stage_steps(m3, a3, st)
    nx2 = NEAREST_2D.get(n, int(round((math.sqrt(L3 ** 3) - 1) / (NB - 1))))
    D2, L2 = lattice_description(nx2)
    m2 = D2.stride * L2
    v2 = vectors(m2, L2, D2.stride)
    a2 = {k: p(t) for k, t in v2.items()}
    lat2, lat4 = steps(lambda name: getattr(L, f"cuddh_hip_wave_lattice_{name}_f64"), C.byref(D2), a2, st)
    inner = 20 if m3 < 2e7 else 5
    t = timed({"box rk2": box2, "stage rk2": stage2, "lattice rk2": lat2, "box rk4": box4, "stage rk4": stage4, "lattice rk4": lat4}, inner)
    say(f"step n={n}^3 elements: {L3}^3 = {L3 ** 3} nodes, {m3} slots ({8 * m3 / 1e6:.1f} MB per vector), tile {L.cuddh_hip_wave_box_tile_x()} x "
        f"{L.cuddh_hip_wave_box_tile_y()} x {L.cuddh_hip_wave_box_tile_z()}; 2-D lattice {nx2}^2 elements: {L2 * L2} nodes, {m2} slots")
    for scheme, sweeps in (("rk2", 2), ("rk4", 4)):
        b, s, l2 = t[f"box {scheme}"], t[f"stage {scheme}"], t[f"lattice {scheme}"]
        rate = lambda ms, slots, vec: vec * 8 * slots / (ms * 1e-3) / 1e12  # noqa: E731
        say(f"  {scheme}: box {1e3 * b[0] / sweeps:8.1f} us per sweep (step min {1e3 * b[1]:.1f} max {1e3 * b[2]:.1f} us) {rate(b[0], m3, VECTORS[scheme]):5.2f} TB/s on "
            f"{VECTORS[scheme]} vectors;  stage alone {1e3 * s[0] / sweeps:8.1f} us per sweep {rate(s[0], m3, VECTORS[scheme] + 1):5.2f} TB/s on {VECTORS[scheme] + 1};  "
            f"box / stage alone {b[0] / s[0]:.3f};  2-D lattice {1e3 * l2[0] / sweeps:8.1f} us per sweep {rate(l2[0], m2, VECTORS[scheme]):5.2f} TB/s, "
            f"per node box / lattice {(b[0] / m3) / (l2[0] / m2):.3f}")
    del v3, v2


def period(n):
    L3 = n * (NB - 1) + 1
    omega = 2 * math.pi * n / 10
    g = torch.Generator(device=dev).manual_seed(2)
    z = torch.randn(2 * L3 ** 3, dtype=torch.float64, device=dev, generator=g)
    out = torch.empty_like(z)
    for scheme, coarsen in (("rk2", None), ("rk4", 4)):
        W = cd.WaveHoltzBox(omega, np.ones(L3 ** 3), shape=(n, n, n), box=((-1, 1),) * 3, n_basis=NB, integrator=scheme, coarsen=coarsen)
        info = W.info()
        W.period(z, None, out)
        torch.cuda.synchronize()
        t = timed({"period": lambda: W.period(z, None, out)}, inner=1)["period"]
        say(f"period n={n}^3 nodes={L3 ** 3} {scheme} nt={info['nt']} ({info['sweeps_per_period']} sweeps) [{info['stiffness_kernel']}]: {t[0]:.2f} ms "
            f"(min {t[1]:.2f} max {t[2]:.2f}) = {1e3 * t[0] / info['sweeps_per_period']:.1f} us per sweep; finite={bool(torch.isfinite(out).all())}")
        del W


def solve(n):
    L3 = n * (NB - 1) + 1
    omega = 2 * math.pi * n / 10
    W = cd.WaveHoltzBox(omega, np.ones(L3 ** 3), shape=(n, n, n), box=((-1, 1),) * 3, n_basis=NB, integrator="rk4", coarsen=4)
    X = W.nodes()
    s = omega * omega / 4
    load = W.mass() * (s / math.pi) ** 1.5 * np.exp(-s * ((X[..., 0] + 0.3) ** 2 + (X[..., 1] - 0.2) ** 2 + (X[..., 2] - 0.1) ** 2))
    f = torch.zeros(W.size(), dtype=torch.float64, device=dev)
    f[:L3 ** 3] = torch.from_numpy(load.reshape(-1)).to(dev)
    del X, load
    b, z = torch.empty_like(f), torch.zeros_like(f)
    W.rhs(f, b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = cd.gmres(W.size(), z, W, b, 20, 400, 1e-4, max_seconds=240.0)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    info = W.info()
    say(f"solve n={n}^3 nodes={L3 ** 3} omega={omega:.2f} a == 1, one Gaussian, rk4/4 nt={info['nt']} GMRES(20) tol 1e-4 [{info['stiffness_kernel']}]: "
        f"success={out.success} matvecs={out.num_matvec} cycles={out.num_iter} rel_res={out.res_norm[-1] / out.res_norm[0]:.3e} seconds={sec:.2f} "
        f"ms_per_period={1e3 * sec / max(1, out.num_matvec):.2f} us_per_sweep={1e6 * sec / max(1, out.num_matvec) / info['sweeps_per_period']:.1f} "
        f"finite={bool(torch.isfinite(z).all())}")


say(f"waveholtz_box_rates.py parts={parts} sizes={sizes} reps={reps} device={torch.cuda.get_device_name(0)}")
for part, fn, which in (("step", step, sizes), ("period", period, period_sizes), ("solve", solve, solve_sizes)):
    if part in parts:
        for n in which:
            fn(n)
            torch.cuda.empty_cache()
