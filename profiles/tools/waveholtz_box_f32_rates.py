"""What the fp32 box sweeps cost beside the fp64 ones on one MI355X, n_basis 4, a == 1, homogeneous form.

step     per size (n^3 elements): us per sweep of cuddh_hip_wave_box32_* and of cuddh_hip_wave_box_*_f64 averaged over an RK2 step
         (rk2_a, rk2_b) and over an RK4 step (rk4_1 .. rk4_4, with the march's ps ping-pong), TB/s on the stated bytes (18 / 46
         vectors of 4 or 8 B per slot and step) and the fp32 / fp64 ratio with its spread.  Both families of the same build are
         measured in the same run, alternating, device events around `inner` back-to-back steps, medians of `reps` after two warm-up
         passes.  The fp64 pointwise stage alone (cuddh_hip_wave_stage_*_f64) on the fp64 length is printed for orientation; there is
         no float stage entry point in the library, so the fp32 stage alone is not measured.
period   ms per homogeneous period of cd.WaveHoltzBox at both precisions, rk2 and rk4 / 4, omega = 2 pi n / 10 on [-1, 1]^3.
solve    one whole solve at both precisions: omega = 2 pi n / 10, a == 1, one Gaussian load, rk4 / 4, GMRES(20), tol 1e-4: matvecs,
         seconds, and the residual of the fp32 solution in the fp64 operator.

  python profiles/tools/waveholtz_box_f32_rates.py [parts=step,period,solve] [sizes=32,64,128] [period_sizes=32,64] [solve_sizes=64] [reps=7] [out=profiles/r35/wave_box_f32_rates.txt]
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
out_path = Path(argv.get("out", str(ROOT / "profiles" / "r35" / "wave_box_f32_rates.txt")))
if not torch.cuda.is_available():
    sys.exit("waveholtz_box_f32_rates.py measures on the GPU: none is visible")
dev = torch.device("cuda:0")
cd.use_torch_stream()
NB = 4
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
    """ms per call of every f in fs (name -> callable): all `reps` values, alternating, after two warm-up passes"""
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
    return times


def vectors(m, Lx, stride, dtype):
    g = torch.Generator(device=dev).manual_seed(1)
    v = {k: torch.randn(m, dtype=dtype, device=dev, generator=g) for k in ("w", "p", "q", "u", "v", "ps", "ps2", "qs", "aq", "ap")}
    v["invm"] = torch.rand(m, dtype=dtype, device=dev, generator=g) + 0.5
    v["Hi"] = torch.zeros(m, dtype=dtype, device=dev)
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
    """the fp64 stages alone on n elements: w is read, not computed"""
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


def box_description(n, rows):
    D, unit = N.WaveBox(), np.array([-1.0, 1.0] * 3)
    N.check_capi(N.lib.cuddh_wave_box_describe_rows(n, n, n, unit.ctypes.data, NB, None, 63, rows, C.byref(D), None, None, None, None, None, None, None))
    return D


def step(n):
    L, st = N.lib, stream()
    L3 = n * (NB - 1) + 1
    D64, D32 = box_description(n, 2), box_description(n, 4)
    m64, m32 = D64.stride * L3 * L3, D32.stride * L3 * L3
    v64, v32 = vectors(m64, L3, D64.stride, torch.float64), vectors(m32, L3, D32.stride, torch.float32)
    a64, a32 = {k: p(t) for k, t in v64.items()}, {k: p(t) for k, t in v32.items()}
    f64_2, f64_4 = steps(lambda name: getattr(L, f"cuddh_hip_wave_box_{name}_f64"), C.byref(D64), a64, st)
    f32_2, f32_4 = steps(lambda name: getattr(L, f"cuddh_hip_wave_box32_{name}"), C.byref(D32), a32, st)
    stage2, stage4 = stage_steps(m64, a64, st)
    inner = 20 if m64 < 2e7 else 5
    t = timed({"f32 rk2": f32_2, "f64 rk2": f64_2, "stage rk2": stage2, "f32 rk4": f32_4, "f64 rk4": f64_4, "stage rk4": stage4}, inner)
    say(f"step n={n}^3 elements: {L3}^3 = {L3 ** 3} nodes; fp32 {m32} slots ({4 * m32 / 1e6:.1f} MB per vector, stride {D32.stride}), tile "
        f"{L.cuddh_hip_wave_box32_tile_x()} x {L.cuddh_hip_wave_box32_tile_y()} x {L.cuddh_hip_wave_box32_tile_z()}; fp64 {m64} slots "
        f"({8 * m64 / 1e6:.1f} MB per vector, stride {D64.stride})")
    for scheme, sweeps in (("rk2", 2), ("rk4", 4)):
        a, b, s = t[f"f32 {scheme}"], t[f"f64 {scheme}"], t[f"stage {scheme}"]
        ma, mb, ms = statistics.median(a), statistics.median(b), statistics.median(s)
        rate = lambda ms_, slots, vec, size: vec * size * slots / (ms_ * 1e-3) / 1e12  # noqa: E731
        ratios = sorted(x / y for x, y in zip(a, b))  # pass by pass: the two were measured next to each other
        say(f"  {scheme}: fp32 {1e3 * ma / sweeps:8.1f} us per sweep (step min {1e3 * min(a):.1f} max {1e3 * max(a):.1f} us) {rate(ma, m32, VECTORS[scheme], 4):5.2f} TB/s on "
            f"{VECTORS[scheme]} vectors of 4 B;  fp64 {1e3 * mb / sweeps:8.1f} us per sweep (step min {1e3 * min(b):.1f} max {1e3 * max(b):.1f} us) "
            f"{rate(mb, m64, VECTORS[scheme], 8):5.2f} TB/s on {VECTORS[scheme]} vectors of 8 B;  fp32 / fp64 {ma / mb:.3f} (per pass {ratios[0]:.3f} .. {ratios[-1]:.3f});  "
            f"fp64 stage alone {1e3 * ms / sweeps:8.1f} us per sweep, fp32 box / fp64 stage alone {ma / ms:.3f}")
    del v64, v32


def period(n):
    L3 = n * (NB - 1) + 1
    omega = 2 * math.pi * n / 10
    g = torch.Generator(device=dev).manual_seed(2)
    z = torch.randn(2 * L3 ** 3, dtype=torch.float64, device=dev, generator=g)
    out = torch.empty_like(z)
    for scheme, coarsen in (("rk2", None), ("rk4", 4)):
        W = {prec: cd.WaveHoltzBox(omega, np.ones(L3 ** 3), shape=(n, n, n), box=((-1, 1),) * 3, n_basis=NB, integrator=scheme, coarsen=coarsen,
                                   precision=prec) for prec in ("f32", "f64")}
        for w in W.values():
            w.period(z, None, out)
        torch.cuda.synchronize()
        t = timed({prec: (lambda w=w: w.period(z, None, out)) for prec, w in W.items()}, inner=1)
        info = W["f32"].info()
        m32, m64 = statistics.median(t["f32"]), statistics.median(t["f64"])
        say(f"period n={n}^3 nodes={L3 ** 3} {scheme} nt={info['nt']} ({info['sweeps_per_period']} sweeps): [{info['stiffness_kernel']}] {m32:.2f} ms "
            f"(min {min(t['f32']):.2f} max {max(t['f32']):.2f}) = {1e3 * m32 / info['sweeps_per_period']:.1f} us per sweep;  [{W['f64'].info()['stiffness_kernel']}] "
            f"{m64:.2f} ms (min {min(t['f64']):.2f} max {max(t['f64']):.2f}) = {1e3 * m64 / info['sweeps_per_period']:.1f} us per sweep;  fp32 / fp64 {m32 / m64:.3f}; "
            f"finite={bool(torch.isfinite(out).all())}")
        del W


def solve(n):
    L3 = n * (NB - 1) + 1
    omega = 2 * math.pi * n / 10
    W = {prec: cd.WaveHoltzBox(omega, np.ones(L3 ** 3), shape=(n, n, n), box=((-1, 1),) * 3, n_basis=NB, integrator="rk4", coarsen=4, precision=prec)
         for prec in ("f64", "f32")}
    X = W["f64"].nodes()
    s = omega * omega / 4
    load = W["f64"].mass() * (s / math.pi) ** 1.5 * np.exp(-s * ((X[..., 0] + 0.3) ** 2 + (X[..., 1] - 0.2) ** 2 + (X[..., 2] - 0.1) ** 2))
    f = torch.zeros(W["f64"].size(), dtype=torch.float64, device=dev)
    f[:L3 ** 3] = torch.from_numpy(load.reshape(-1)).to(dev)
    del X, load
    b64 = torch.empty_like(f)
    W["f64"].rhs(f, b64)
    for prec, w in W.items():
        b, z = torch.empty_like(f), torch.zeros_like(f)
        w.rhs(f, b)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = cd.gmres(w.size(), z, w, b, 20, 400, 1e-4, max_seconds=240.0)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        info = w.info()
        y = torch.empty_like(f)
        W["f64"].action(z, y)  # the residual of this solution in the fp64 operator
        res64 = float(torch.linalg.norm(b64 - y) / torch.linalg.norm(b64))
        say(f"solve n={n}^3 nodes={L3 ** 3} omega={omega:.2f} a == 1, one Gaussian, rk4/4 nt={info['nt']} GMRES(20) tol 1e-4 [{info['stiffness_kernel']}]: "
            f"success={out.success} matvecs={out.num_matvec} cycles={out.num_iter} rel_res={out.res_norm[-1] / out.res_norm[0]:.3e} seconds={sec:.2f} "
            f"ms_per_period={1e3 * sec / max(1, out.num_matvec):.2f} us_per_sweep={1e6 * sec / max(1, out.num_matvec) / info['sweeps_per_period']:.1f} "
            f"residual_in_the_fp64_operator={res64:.3e} finite={bool(torch.isfinite(z).all())}")
        del b, z, y


say(f"waveholtz_box_f32_rates.py parts={parts} sizes={sizes} reps={reps} device={torch.cuda.get_device_name(0)}")
for part, fn, which in (("step", step, sizes), ("period", period, period_sizes), ("solve", solve, solve_sizes)):
    if part in parts:
        for n in which:
            fn(n)
            torch.cuda.empty_cache()
