"""What the whole-domain WaveHoltz march costs on one MI355X, n_basis 4, a == 1, omega = 2 pi nx / 10.

stages   us of every cuddh_hip_wave_stage_* launch (homogeneous form: the GMRES action) and of the stiffness apply it follows,
         beside cuddh_hip_axpby_f64 at the same n, alternating in the same run, device events around `inner` back-to-back
         launches, median of `reps`.  TB/s on the stated bytes: 8 B per vector read or written per dof (begin 6, rk2_a 7, rk2_b 12,
         rk4_1 9, rk4_2 / rk4_3 12, rk4_4 14 vectors; axpby 3).  us per sweep = stiffness apply + stage, averaged over a step.
period   ms of WaveHoltz.period (one launch per sweep besides the apply) against the same march composed from the entry points the
         library had before (cuddh_operator_apply, cuddh_hip_copy_f64, cuddh_hip_diag_scale_f64, cuddh_hip_axpby_f64: 10 launches
         per RK2 step besides the two applies), alternating in the same run; the two results are compared first.
solve    one whole solve per size in the example's regime (the disk coefficient, the Gaussians as load, GMRES(20), tol 1e-4),
         rk4 / coarsen 4: matvecs (= periods) and seconds of the gmres() call, beside DDH's figures for the same problems
         (DESIGN 5.2).

lattice  (parts lattice_stages, lattice_period, lattice_solve; written for profiles/r25/wave_lattice_rates.txt) the same for
         sweep="lattice" (csrc/kernels/wave_lattice.hip): us of every cuddh_hip_wave_lattice_* launch beside the operator
         form's stage and its Gauss stiffness apply and beside axpby, alternating in one run; TB/s on 8 B per vector read or
         written per lattice slot (rk2_a 6, rk2_b 12, rk4_1 8, rk4_2 / rk4_3 12, rk4_4 14 vectors); ms per homogeneous period and us
         per sweep of sweep="lattice" against sweep="operator" with stiffness "lobatto" and "gauss", rk2 and rk4 / 4, alternating;
         one whole solve in the example's regime with sweep="lattice".

lattice32 (parts lattice32_stages, lattice32_period, lattice32_solve; written for profiles/r26/wave_lattice_f32_rates.txt) precision="f32"
         beside the f64 lattice form of the same build, alternating in one run (csrc/kernels/wave_lattice_f32.hip): us of
         every cuddh_hip_wave32_* launch beside its cuddh_hip_wave_lattice_*_f64 twin, and axpby_f32 beside axpby_f64; TB/s on 4 B
         (f32) or 8 B (f64) per vector read or written per lattice slot, the vector counts above; ms per homogeneous period and us
         per sweep of both precisions, rk2 and rk4 / 4, and how far the two results are apart; the example-regime solve at both
         precisions: matvecs, seconds, and the residual of the f32 solution in the f64 operator.

pair     (parts pair_step, pair_period, pair_solve; written for profiles/r27/wave_pair_rates.txt) launch="pair" beside launch="sweep" of the
         same build, alternating in one run (csrc/kernels/wave_pair.hip, wave_pair_f32.hip), fp64 and fp32, rk2 and rk4:
         us per time step from the entry points (homogeneous form; two or four one-sweep launches against one or two paired ones,
         the paired ones with the march's buffer swaps) and TB/s on the stated vectors (rk2 18 / 10, rk4 46 / 22 per slot and step);
         ms per homogeneous period of the two solvers, whose results must be torch.equal; the example-regime solve with both.  The
         byte model expects paired / per-sweep = 0.56 (rk2) and 0.48 (rk4).

cells    (parts cells_step, cells_solve; written for profiles/r29/wave_cells_rates.txt) the sweeps on a grid with missing cells
         (csrc/kernels/wave_cells.hip, wave_cells_f32.hip) beside the full-rectangle lattice sweeps of the same build,
         alternating in one run, fp64 and fp32, rk2 and rk4: us per time step from the entry points (homogeneous form) of
         cuddh_hip_wave_lattice_* / wave32_*, of cuddh_hip_wave_cells_* with every cell present (what the flags cost) and with the
         upper right quadrant of cells removed (what void tiles cost); one solve in the example's regime (disk coefficient,
         Gaussians, GMRES(20), 1e-4, rk4 / 4) with a sound-hard square obstacle of nx / 8 x nx / 8 cells at [0.25, 0.5]^2, sweep
         "lattice" in fp64 and fp32 against sweep "operator" with stiffness "lobatto" on the same mesh: matvecs and seconds.

weights  (parts weights_step, weights_solve; written for profiles/r30/wave_weights_rates.txt) the sweeps with a per-cell stiffness
         weight (csrc/kernels/wave_weights.hip, wave_weights_f32.hip) beside the sweeps of the same build, alternating
         in one run, fp64 and fp32, rk2 and rk4: us per time step from the entry points (homogeneous form) of
         cuddh_hip_wave_weights_* on an all-ones weight array, of cuddh_hip_wave_cells_* on all-ones flags and of
         cuddh_hip_wave_lattice_* / wave32_* (what the real-valued weights cost); one solve in the example's regime (disk
         coefficient, Gaussians, GMRES(20), 1e-4, rk4 / 4, every boundary edge absorbing) with an inclusion of beta = 4 on nx / 8 x
         nx / 8 cells at [0.25, 0.5]^2 (time ratio 1, as the example has it for its disk of a = 0.2), in fp64 and fp32, and the
         same solve at beta == 1 on wave_lattice: matvecs and seconds.

  python profiles/tools/waveholtz_rates.py [parts=stages,period,solve] [sizes=256,512,1024] [solve_sizes=256,512] [reps=7] [out=profiles/r24/waveholtz_rates.txt]
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
parts = argv.get("parts", "stages,period,solve").split(",")
sizes = [int(v) for v in argv.get("sizes", "256,512,1024").split(",")]
solve_sizes = [int(v) for v in argv.get("solve_sizes", "256,512").split(",") if v]
reps = int(argv.get("reps", "7"))
out_path = Path(argv.get("out", str(ROOT / "profiles" / "r24" / "waveholtz_rates.txt")))
if not torch.cuda.is_available():
    sys.exit("waveholtz_rates.py measures on the GPU: none is visible")
dev = torch.device("cuda:0")
cd.use_torch_stream()
NB = 4
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


def space(nx):
    mesh = cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0)
    return mesh, cd.H1Space(mesh, cd.Basis(NB))


STAGE_VECTORS = {"begin": 6, "rk2_a": 7, "rk2_b": 12, "rk4_1": 9, "rk4_2": 12, "rk4_3": 12, "rk4_4": 14, "axpby": 3}


def stages(nx):
    mesh, fem = space(nx)
    n = fem.size()
    g = torch.Generator(device=dev).manual_seed(1)
    v = {k: torch.randn(n, dtype=torch.float64, device=dev, generator=g) for k in ("w", "p", "q", "u", "v", "ps", "qs", "aq", "ap", "zu", "zv")}
    v["invm"] = torch.rand(n, dtype=torch.float64, device=dev, generator=g) + 0.5
    v["Hi"] = torch.zeros(n, dtype=torch.float64, device=dev)
    K = cd.StiffnessMatrix(fem)
    K.action(v["p"], v["w"])
    L, st = N.lib, stream()
    dt = 1e-6  # (the timed launches repeat on the same vectors: keep them bounded)
    a = {k: p(t) for k, t in v.items()}
    fs = {
        "stiffness": lambda: K.action(v["p"], v["w"]),
        "begin": lambda: N.check(L.cuddh_hip_wave_stage_begin_f64(n, 0.5, a["zu"], a["zv"], a["p"], a["q"], a["u"], a["v"], st)),
        "rk2_a": lambda: N.check(L.cuddh_hip_wave_stage_rk2_a_f64(n, dt / 2, 1.0, 0.0, a["w"], a["p"], a["q"], a["invm"], a["Hi"], None, None, a["qs"], a["ps"], st)),
        "rk2_b": lambda: N.check(L.cuddh_hip_wave_stage_rk2_b_f64(n, dt, 1.0, 0.0, 1e-3, a["w"], a["qs"], a["invm"], a["Hi"], None, None, a["p"], a["q"], a["u"], a["v"], st)),
        "rk4_1": lambda: N.check(L.cuddh_hip_wave_stage_rk4_1_f64(n, dt / 2, 1.0, 0.0, a["w"], a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps"], a["qs"], a["aq"], a["ap"], st)),
        "rk4_2": lambda: N.check(L.cuddh_hip_wave_stage_rk4_2_f64(n, dt / 2, 1.0, 0.0, a["w"], a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps"], a["qs"], a["aq"], a["ap"], st)),
        "rk4_3": lambda: N.check(L.cuddh_hip_wave_stage_rk4_3_f64(n, dt, 1.0, 0.0, a["w"], a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps"], a["qs"], a["aq"], a["ap"], st)),
        "rk4_4": lambda: N.check(L.cuddh_hip_wave_stage_rk4_4_f64(n, dt / 6, 1.0, 0.0, 1e-3, a["w"], a["qs"], a["aq"], a["ap"], a["invm"], a["Hi"], None, None, a["p"], a["q"], a["u"], a["v"], st)),
        "axpby": lambda: N.check(L.cuddh_hip_axpby_f64(n, 1e-6, a["zu"], 1.0, a["zv"], st)),
    }
    t = timed(fs, inner=20)
    say(f"stages nx={nx} ndof={n} ({8 * n / 1e6:.1f} MB per vector) stiffness kernel {K.kernel()!r}")
    ax = STAGE_VECTORS["axpby"] * 8 * n / (t["axpby"][0] * 1e-3) / 1e12
    for k, (med, lo, hi) in t.items():
        if k == "stiffness":
            say(f"  {k:10s} {1e3 * med:8.1f} us (min {1e3 * lo:.1f} max {1e3 * hi:.1f})")
        else:
            rate = STAGE_VECTORS[k] * 8 * n / (med * 1e-3) / 1e12
            say(f"  {k:10s} {1e3 * med:8.1f} us (min {1e3 * lo:.1f} max {1e3 * hi:.1f})  {STAGE_VECTORS[k]:2d} vectors  {rate:5.2f} TB/s  {rate / ax:4.2f} of axpby")
    s = t["stiffness"][0]
    say(f"  us per sweep: rk2 {1e3 * (s + (t['rk2_a'][0] + t['rk2_b'][0]) / 2):.1f} (apply {1e3 * s:.1f} + stage {1e3 * (t['rk2_a'][0] + t['rk2_b'][0]) / 2:.1f}), "
        f"rk4 {1e3 * (s + sum(t[k][0] for k in ('rk4_1', 'rk4_2', 'rk4_3', 'rk4_4')) / 4):.1f} "
        f"(apply {1e3 * s:.1f} + stage {1e3 * sum(t[k][0] for k in ('rk4_1', 'rk4_2', 'rk4_3', 'rk4_4')) / 4:.1f})")


def composed_period(W, K, z, out, tab, work):
    """the homogeneous RK2 period from the entry points the library had before the stage kernels"""
    L, st = N.lib, stream()
    n = z.numel() // 2
    nt, dt, filt = tab
    w, pp, q, u, v, ph, qh, invm, Hi = (p(work[k]) for k in ("w", "p", "q", "u", "v", "ph", "qh", "invm", "Hi"))
    zu, zv = C.c_void_p(z.data_ptr()), C.c_void_p(z.data_ptr() + 8 * n)
    for src, dst in ((zu, pp), (zv, q), (zu, u), (zv, v)):
        L.cuddh_hip_copy_f64(n, src, dst, st)
    L.cuddh_hip_axpby_f64(n, 0.0, pp, filt[0], u, st)
    L.cuddh_hip_axpby_f64(n, 0.0, q, filt[0], v, st)
    for it in range(1, nt + 1):
        L.cuddh_operator_apply(K._h, pp, w)
        L.cuddh_hip_diag_scale_f64(n, 1, -1.0, Hi, q, w, st)          # w -= Hi q
        L.cuddh_hip_copy_f64(n, q, qh, st)
        L.cuddh_hip_diag_scale_f64(n, 1, 0.5 * dt, invm, w, qh, st)   # qh = q + dt/2 invm w
        L.cuddh_hip_copy_f64(n, pp, ph, st)
        L.cuddh_hip_axpby_f64(n, -0.5 * dt, q, 1.0, ph, st)           # ph = p - dt/2 q
        L.cuddh_operator_apply(K._h, ph, w)
        L.cuddh_hip_diag_scale_f64(n, 1, -1.0, Hi, qh, w, st)         # w -= Hi qh
        L.cuddh_hip_axpby_f64(n, -dt, qh, 1.0, pp, st)                # p -= dt qh
        L.cuddh_hip_diag_scale_f64(n, 1, dt, invm, w, q, st)          # q += dt invm w
        L.cuddh_hip_axpby_f64(n, filt[it], pp, 1.0, u, st)
        L.cuddh_hip_axpby_f64(n, filt[it], q, 1.0, v, st)
    L.cuddh_hip_copy_f64(n, u, C.c_void_p(out.data_ptr()), st)
    L.cuddh_hip_copy_f64(n, v, C.c_void_p(out.data_ptr() + 8 * n), st)


def period(nx):
    mesh, fem = space(nx)
    n = fem.size()
    omega = 2 * math.pi * nx / 10
    W = cd.WaveHoltz(omega, np.ones(n), fem)
    info = W.info()
    nt, dt = info["nt"], info["dt"]
    filt = [dt * (omega / math.pi) * (math.cos(omega * k * dt) - 0.25) for k in range(nt + 1)]
    filt[0] *= 0.5
    filt[nt] *= 0.5
    g = torch.Generator(device=dev).manual_seed(2)
    z = torch.randn(2 * n, dtype=torch.float64, device=dev, generator=g)
    a, b = torch.empty_like(z), torch.empty_like(z)
    K = cd.StiffnessMatrix(fem)
    work = {k: torch.zeros(n, dtype=torch.float64, device=dev) for k in ("w", "p", "q", "u", "v", "ph", "qh", "Hi")}
    # the same lumped matrices as the solver's: 1 / m through the library, h a on the boundary through the face space
    ones = torch.ones(n, dtype=torch.float64, device=dev)
    work["invm"] = torch.empty_like(ones)
    cd.DiagInvMassMatrix(fem).action(ones, work["invm"])
    fs = cd.FaceSpace(fem, mesh.boundary_edges())
    hf = torch.ones(fs.size(), dtype=torch.float64, device=dev)
    inv_h = torch.empty_like(hf)
    cd.DiagInvFaceMassMatrix(fs).action(hf, inv_h)
    fs.prolong(1.0 / inv_h, work["Hi"])
    W.period(z, None, a)
    composed_period(W, K, z, b, (nt, dt, filt), work)
    torch.cuda.synchronize()
    diff = float(torch.linalg.norm(a - b) / torch.linalg.norm(a))
    t = timed({"fused": lambda: W.period(z, None, a), "composed": lambda: composed_period(W, K, z, b, (nt, dt, filt), work)}, inner=1)
    f, c = t["fused"], t["composed"]
    say(f"period nx={nx} ndof={n} rk2 nt={nt} ({2 * nt} sweeps): fused {f[0]:.2f} ms (min {f[1]:.2f} max {f[2]:.2f}) = {1e3 * f[0] / (2 * nt):.1f} us per sweep; "
        f"composed {c[0]:.2f} ms (min {c[1]:.2f} max {c[2]:.2f}) = {1e3 * c[0] / (2 * nt):.1f} us per sweep; fused / composed {f[0] / c[0]:.3f}; results differ by {diff:.1e}")


DDH_FIGURES = {256: "390 matvecs", 512: "1,887 matvecs in 25 s", 1024: "GMRES(20) stalls at 3.3e-3 (11,593 matvecs); GMRES(200) at 4.6e-4 after 910 s"}


def solve(nx):
    mesh, fem = space(nx)
    n = fem.size()
    omega = 2 * math.pi * nx / 10
    f = torch.zeros(2 * n, dtype=torch.float64, device=dev)
    a = torch.zeros(n, dtype=torch.float64, device=dev)
    cd.linear_functional(fem, cd.GAUSSIANS, f[:n], param=omega)
    cd.linear_functional(fem, cd.ALPHA_DISK, a)
    cd.DiagInvMassMatrix(fem).action(a, a)
    W = cd.WaveHoltz(omega, a.cpu().numpy(), fem, integrator="rk4", coarsen=4)
    b, z = torch.empty_like(f), torch.zeros_like(f)
    W.rhs(f, b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = cd.gmres(2 * n, z, W, b, 20, 400, 1e-4, max_seconds=900.0)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    info = W.info()
    rel = out.res_norm[-1] / out.res_norm[0]
    say(f"solve nx={nx} ndof={n} omega={omega:.2f} disk coefficient (min a {float(a.min()):.3f}) rk4/4 nt={info['nt']} GMRES(20) tol 1e-4: success={out.success} "
        f"matvecs={out.num_matvec} cycles={out.num_iter} rel_res={rel:.3e} seconds={sec:.2f} ms_per_period={1e3 * sec / max(1, out.num_matvec):.2f} "
        f"us_per_sweep={1e6 * sec / max(1, out.num_matvec) / info['sweeps_per_period']:.1f} finite={bool(torch.isfinite(z).all())}; DDH (DESIGN 5.2): {DDH_FIGURES.get(nx, 'not recorded')}")


LATTICE_VECTORS = {"rk2_a": 6, "rk2_b": 12, "rk4_1": 8, "rk4_2": 12, "rk4_3": 12, "rk4_4": 14}


def lattice_stages(nx):
    mesh, fem = space(nx)
    n = fem.size()
    Lx = nx * (NB - 1) + 1
    D = N.WaveLattice()
    D.nx, D.ny, D.n_basis, D.stride, D.cx, D.cy = nx, nx, NB, Lx + Lx % 2, 1.0, 1.0
    A, w, basis = np.zeros((NB, NB)), np.zeros(NB), cd.Basis(NB)
    N.check_capi(N.lib.cuddh_wave_lattice_tables(basis._h, A.ctypes.data, w.ctypes.data))
    for i, x in enumerate(A.reshape(-1)):
        D.A[i] = x
    for i, x in enumerate(w):
        D.w[i] = x
    m = D.stride * Lx  # slots of a lattice vector
    g = torch.Generator(device=dev).manual_seed(1)
    names = ("w", "p", "q", "u", "v", "ps", "ps2", "qs", "aq", "ap", "zu", "zv")
    v = {k: torch.randn(m, dtype=torch.float64, device=dev, generator=g) for k in names}
    v["invm"] = torch.rand(m, dtype=torch.float64, device=dev, generator=g) + 0.5
    v["Hi"] = torch.zeros(m, dtype=torch.float64, device=dev)
    if D.stride > Lx:  # the padding column: zero state, invm = 0
        for t in v.values():
            t.view(Lx, D.stride)[:, Lx:] = 0.0
    K = cd.StiffnessMatrix(fem)
    K.action(v["p"][:n], v["w"][:n])
    L, st, d = N.lib, stream(), C.byref(D)
    dt = 1e-9  # (the timed launches repeat on the same vectors: keep them bounded)
    a = {k: p(t) for k, t in v.items()}
    fs = {
        "stiffness": lambda: K.action(v["p"][:n], v["w"][:n]),
        "axpby": lambda: N.check(L.cuddh_hip_axpby_f64(m, 1e-6, a["zu"], 1.0, a["zv"], st)),
        "stage rk2_a": lambda: N.check(L.cuddh_hip_wave_stage_rk2_a_f64(n, dt / 2, 1.0, 0.0, a["w"], a["p"], a["q"], a["invm"], a["Hi"], None, None, a["qs"], a["ps"], st)),
        "lattice rk2_a": lambda: N.check(L.cuddh_hip_wave_lattice_rk2_a_f64(d, dt / 2, 1.0, 0.0, a["p"], a["q"], a["invm"], a["Hi"], None, None, a["qs"], a["ps"], st)),
        "stage rk2_b": lambda: N.check(L.cuddh_hip_wave_stage_rk2_b_f64(n, dt, 1.0, 0.0, 1e-3, a["w"], a["qs"], a["invm"], a["Hi"], None, None, a["p"], a["q"], a["u"], a["v"], st)),
        "lattice rk2_b": lambda: N.check(L.cuddh_hip_wave_lattice_rk2_b_f64(d, dt, 1.0, 0.0, 1e-3, a["ps"], a["qs"], a["invm"], a["Hi"], None, None, a["p"], a["q"], a["u"], a["v"], st)),
        "stage rk4_1": lambda: N.check(L.cuddh_hip_wave_stage_rk4_1_f64(n, dt / 2, 1.0, 0.0, a["w"], a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps"], a["qs"], a["aq"], a["ap"], st)),
        "lattice rk4_1": lambda: N.check(L.cuddh_hip_wave_lattice_rk4_1_f64(d, dt / 2, 1.0, 0.0, a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps"], a["qs"], a["aq"], a["ap"], st)),
        "stage rk4_2": lambda: N.check(L.cuddh_hip_wave_stage_rk4_2_f64(n, dt / 2, 1.0, 0.0, a["w"], a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps"], a["qs"], a["aq"], a["ap"], st)),
        "lattice rk4_2": lambda: N.check(L.cuddh_hip_wave_lattice_rk4_2_f64(d, dt / 2, 1.0, 0.0, a["ps"], a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps2"], a["qs"], a["aq"], a["ap"], st)),
        "lattice rk4_3": lambda: N.check(L.cuddh_hip_wave_lattice_rk4_3_f64(d, dt, 1.0, 0.0, a["ps2"], a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps"], a["qs"], a["aq"], a["ap"], st)),
        "stage rk4_4": lambda: N.check(L.cuddh_hip_wave_stage_rk4_4_f64(n, dt / 6, 1.0, 0.0, 1e-3, a["w"], a["qs"], a["aq"], a["ap"], a["invm"], a["Hi"], None, None, a["p"], a["q"], a["u"], a["v"], st)),
        "lattice rk4_4": lambda: N.check(L.cuddh_hip_wave_lattice_rk4_4_f64(d, dt / 6, 1.0, 0.0, 1e-3, a["ps"], a["qs"], a["aq"], a["ap"], a["invm"], a["Hi"], None, None, a["p"], a["q"], a["u"], a["v"], st)),
    }
    t = timed(fs, inner=20)
    say(f"lattice stages nx={nx} ndof={n} slots={m} ({8 * m / 1e6:.1f} MB per vector) tile {L.cuddh_hip_wave_lattice_tile_x()} x {L.cuddh_hip_wave_lattice_tile_y()}; "
        f"operator form: stiffness kernel {K.kernel()!r}")
    ax = STAGE_VECTORS["axpby"] * 8 * m / (t["axpby"][0] * 1e-3) / 1e12
    for k, (med, lo, hi) in t.items():
        vectors = LATTICE_VECTORS[k.split()[1]] if k.startswith("lattice") else (STAGE_VECTORS[k.split()[1]] if k.startswith("stage") else STAGE_VECTORS.get(k))
        if vectors is None:
            say(f"  {k:14s} {1e3 * med:8.1f} us (min {1e3 * lo:.1f} max {1e3 * hi:.1f})")
        else:
            rate = vectors * 8 * (m if not k.startswith("stage") else n) / (med * 1e-3) / 1e12
            say(f"  {k:14s} {1e3 * med:8.1f} us (min {1e3 * lo:.1f} max {1e3 * hi:.1f})  {vectors:2d} vectors  {rate:5.2f} TB/s  {rate / ax:4.2f} of axpby")
    s = t["stiffness"][0]
    lat2 = (t["lattice rk2_a"][0] + t["lattice rk2_b"][0]) / 2
    lat4 = sum(t[f"lattice {k}"][0] for k in ("rk4_1", "rk4_2", "rk4_3", "rk4_4")) / 4
    op2 = (t["stage rk2_a"][0] + t["stage rk2_b"][0]) / 2
    op4 = (t["stage rk4_1"][0] + 2 * t["stage rk4_2"][0] + t["stage rk4_4"][0]) / 4
    say(f"  us per sweep: rk2 lattice {1e3 * lat2:.1f}, operator/gauss {1e3 * (s + op2):.1f} (apply {1e3 * s:.1f} + stage {1e3 * op2:.1f}); "
        f"rk4 lattice {1e3 * lat4:.1f}, operator/gauss {1e3 * (s + op4):.1f} (apply {1e3 * s:.1f} + stage {1e3 * op4:.1f})")


def lattice_period(nx):
    mesh, fem = space(nx)
    n = fem.size()
    omega = 2 * math.pi * nx / 10
    g = torch.Generator(device=dev).manual_seed(2)
    z = torch.randn(2 * n, dtype=torch.float64, device=dev, generator=g)
    for scheme, coarsen in (("rk2", None), ("rk4", 4)):
        Ws = {"lattice": cd.WaveHoltz(omega, np.ones(n), fem, integrator=scheme, coarsen=coarsen, stiffness="lobatto", sweep="lattice"),
              "operator/lobatto": cd.WaveHoltz(omega, np.ones(n), fem, integrator=scheme, coarsen=coarsen, stiffness="lobatto"),
              "operator/gauss": cd.WaveHoltz(omega, np.ones(n), fem, integrator=scheme, coarsen=coarsen)}
        out = {k: torch.empty_like(z) for k in Ws}
        for k, W in Ws.items():
            W.period(z, None, out[k])
        torch.cuda.synchronize()
        diff = float(torch.linalg.norm(out["lattice"] - out["operator/lobatto"]) / torch.linalg.norm(out["lattice"]))
        sweeps = Ws["lattice"].info()["sweeps_per_period"]
        t = timed({k: (lambda W=W, k=k: W.period(z, None, out[k])) for k, W in Ws.items()}, inner=1)
        text = "; ".join(f"{k} {t[k][0]:.2f} ms (min {t[k][1]:.2f} max {t[k][2]:.2f}) = {1e3 * t[k][0] / sweeps:.1f} us per sweep [{Ws[k].info()['stiffness_kernel']}]" for k in Ws)
        say(f"lattice period nx={nx} ndof={n} {scheme} nt={Ws['lattice'].info()['nt']} ({sweeps} sweeps): {text}; lattice / gauss "
            f"{t['lattice'][0] / t['operator/gauss'][0]:.3f}, lattice / lobatto {t['lattice'][0] / t['operator/lobatto'][0]:.3f}; lattice and operator/lobatto differ by {diff:.1e}")
        del Ws, out


def lattice_solve(nx):
    mesh, fem = space(nx)
    n = fem.size()
    omega = 2 * math.pi * nx / 10
    f = torch.zeros(2 * n, dtype=torch.float64, device=dev)
    a = torch.zeros(n, dtype=torch.float64, device=dev)
    cd.linear_functional(fem, cd.GAUSSIANS, f[:n], param=omega)
    cd.linear_functional(fem, cd.ALPHA_DISK, a)
    cd.DiagInvMassMatrix(fem).action(a, a)
    W = cd.WaveHoltz(omega, a.cpu().numpy(), fem, integrator="rk4", coarsen=4, stiffness="lobatto", sweep="lattice")
    b, z = torch.empty_like(f), torch.zeros_like(f)
    W.rhs(f, b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = cd.gmres(2 * n, z, W, b, 20, 400, 1e-4, max_seconds=600.0)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    info = W.info()
    say(f"lattice solve nx={nx} ndof={n} omega={omega:.2f} disk coefficient rk4/4 nt={info['nt']} GMRES(20) tol 1e-4 sweep=lattice [{info['stiffness_kernel']}]: "
        f"success={out.success} matvecs={out.num_matvec} cycles={out.num_iter} rel_res={out.res_norm[-1] / out.res_norm[0]:.3e} seconds={sec:.2f} "
        f"ms_per_period={1e3 * sec / max(1, out.num_matvec):.2f} us_per_sweep={1e6 * sec / max(1, out.num_matvec) / info['sweeps_per_period']:.1f} "
        f"finite={bool(torch.isfinite(z).all())}; operator/gauss (profiles/r24/waveholtz_rates.txt): "
        f"{ {256: '256 matvecs, 5.15 s', 512: '499 matvecs, 24.58 s', 1024: '985 matvecs, 173.87 s'}.get(nx, 'not recorded')}")


def lattice_description(nx, multiple):
    """the cuddh_wave_lattice of nx x nx elements on [-1, 1]^2 with rows of a multiple of `multiple` elements"""
    Lx = nx * (NB - 1) + 1
    D = N.WaveLattice()
    D.nx, D.ny, D.n_basis, D.stride, D.cx, D.cy = nx, nx, NB, -(-Lx // multiple) * multiple, 1.0, 1.0
    A, w, basis = np.zeros((NB, NB)), np.zeros(NB), cd.Basis(NB)
    N.check_capi(N.lib.cuddh_wave_lattice_tables(basis._h, A.ctypes.data, w.ctypes.data))
    for i, x in enumerate(A.reshape(-1)):
        D.A[i] = x
    for i, x in enumerate(w):
        D.w[i] = x
    return D, Lx


def lattice32_stages(nx):
    L, st = N.lib, stream()
    dt = 1e-9  # (the timed launches repeat on the same vectors: keep them bounded)
    fs, slots = {}, {}
    keep = []
    for tag, dtype, multiple in (("f64", torch.float64, 2), ("f32", torch.float32, 4)):
        D, Lx = lattice_description(nx, multiple)
        m = D.stride * Lx
        slots[tag] = m
        g = torch.Generator(device=dev).manual_seed(1)
        v = {k: torch.randn(m, dtype=dtype, device=dev, generator=g) for k in ("p", "q", "u", "v", "ps", "ps2", "qs", "aq", "ap", "zu", "zv")}
        v["invm"] = torch.rand(m, dtype=dtype, device=dev, generator=g) + 0.5
        v["Hi"] = torch.zeros(m, dtype=dtype, device=dev)
        if D.stride > Lx:  # the padding columns: zero state, invm = 0
            for t in v.values():
                t.view(Lx, D.stride)[:, Lx:] = 0.0
        a, d = {k: p(t) for k, t in v.items()}, C.byref(D)
        keep.append((D, v))
        fn = (lambda name: getattr(L, f"cuddh_hip_wave_lattice_{name}_f64")) if tag == "f64" else (lambda name: getattr(L, f"cuddh_hip_wave32_{name}"))
        axpby = L.cuddh_hip_axpby_f64 if tag == "f64" else L.cuddh_hip_axpby_f32
        fs[f"axpby {tag}"] = lambda a=a, m=m, axpby=axpby: N.check(axpby(m, 1e-6, a["zu"], 1.0, a["zv"], st))
        fs[f"rk2_a {tag}"] = lambda a=a, d=d, fn=fn: N.check(fn("rk2_a")(d, dt / 2, 1.0, 0.0, a["p"], a["q"], a["invm"], a["Hi"], None, None, a["qs"], a["ps"], st))
        fs[f"rk2_b {tag}"] = lambda a=a, d=d, fn=fn: N.check(fn("rk2_b")(d, dt, 1.0, 0.0, 1e-3, a["ps"], a["qs"], a["invm"], a["Hi"], None, None, a["p"], a["q"], a["u"], a["v"], st))
        fs[f"rk4_1 {tag}"] = lambda a=a, d=d, fn=fn: N.check(fn("rk4_1")(d, dt / 2, 1.0, 0.0, a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps"], a["qs"], a["aq"], a["ap"], st))
        fs[f"rk4_2 {tag}"] = lambda a=a, d=d, fn=fn: N.check(fn("rk4_2")(d, dt / 2, 1.0, 0.0, a["ps"], a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps2"], a["qs"], a["aq"], a["ap"], st))
        fs[f"rk4_3 {tag}"] = lambda a=a, d=d, fn=fn: N.check(fn("rk4_3")(d, dt, 1.0, 0.0, a["ps2"], a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps"], a["qs"], a["aq"], a["ap"], st))
        fs[f"rk4_4 {tag}"] = lambda a=a, d=d, fn=fn: N.check(fn("rk4_4")(d, dt / 6, 1.0, 0.0, 1e-3, a["ps"], a["qs"], a["aq"], a["ap"], a["invm"], a["Hi"], None, None, a["p"], a["q"], a["u"], a["v"], st))
    fs = {f"{k} {tag}": fs[f"{k} {tag}"] for k in ("axpby", *LATTICE_VECTORS) for tag in ("f64", "f32")}  # twins side by side
    t = timed(fs, inner=20)
    say(f"lattice32 stages nx={nx} slots f64 {slots['f64']} ({8 * slots['f64'] / 1e6:.1f} MB per vector), f32 {slots['f32']} ({4 * slots['f32'] / 1e6:.1f} MB per vector); "
        f"tiles f64 {L.cuddh_hip_wave_lattice_tile_x()} x {L.cuddh_hip_wave_lattice_tile_y()}, f32 {L.cuddh_hip_wave32_tile_x()} x {L.cuddh_hip_wave32_tile_y()}")
    size = {"f64": 8, "f32": 4}
    for k in ("axpby", *LATTICE_VECTORS):
        vectors = LATTICE_VECTORS.get(k, STAGE_VECTORS["axpby"])
        text = []
        for tag in ("f64", "f32"):
            med, lo, hi = t[f"{k} {tag}"]
            text.append(f"{tag} {1e3 * med:8.1f} us (min {1e3 * lo:.1f} max {1e3 * hi:.1f}) {vectors * size[tag] * slots[tag] / (med * 1e-3) / 1e12:5.2f} TB/s")
        say(f"  {k:6s} {vectors:2d} vectors  " + "   ".join(text) + f"   f32 / f64 time {t[f'{k} f32'][0] / t[f'{k} f64'][0]:.3f}")
    for scheme, names in (("rk2", ("rk2_a", "rk2_b")), ("rk4", ("rk4_1", "rk4_2", "rk4_3", "rk4_4"))):
        per = {tag: sum(t[f"{k} {tag}"][0] for k in names) / len(names) for tag in ("f64", "f32")}
        say(f"  us per sweep {scheme}: f64 {1e3 * per['f64']:.1f}, f32 {1e3 * per['f32']:.1f}, f32 / f64 {per['f32'] / per['f64']:.3f}")
    del keep


def lattice32_period(nx):
    mesh, fem = space(nx)
    n = fem.size()
    omega = 2 * math.pi * nx / 10
    g = torch.Generator(device=dev).manual_seed(2)
    z = torch.randn(2 * n, dtype=torch.float64, device=dev, generator=g)
    for scheme, coarsen in (("rk2", None), ("rk4", 4)):
        Ws = {tag: cd.WaveHoltz(omega, np.ones(n), fem, integrator=scheme, coarsen=coarsen, stiffness="lobatto", sweep="lattice", precision=tag)
              for tag in ("f64", "f32")}
        out = {k: torch.empty_like(z) for k in Ws}
        for k, W in Ws.items():
            W.period(z, None, out[k])
        torch.cuda.synchronize()
        diff = float(torch.linalg.norm(out["f32"] - out["f64"]) / torch.linalg.norm(out["f64"]))
        sweeps = Ws["f64"].info()["sweeps_per_period"]
        t = timed({k: (lambda W=W, k=k: W.period(z, None, out[k])) for k, W in Ws.items()}, inner=1)
        text = "; ".join(f"{k} {t[k][0]:.2f} ms (min {t[k][1]:.2f} max {t[k][2]:.2f}) = {1e3 * t[k][0] / sweeps:.1f} us per sweep [{Ws[k].info()['stiffness_kernel']}]" for k in Ws)
        say(f"lattice32 period nx={nx} ndof={n} {scheme} nt={Ws['f64'].info()['nt']} ({sweeps} sweeps): {text}; f32 / f64 {t['f32'][0] / t['f64'][0]:.3f}; "
            f"the two periods differ by {diff:.2e}")
        del Ws, out


def lattice32_solve(nx):
    mesh, fem = space(nx)
    n = fem.size()
    omega = 2 * math.pi * nx / 10
    f = torch.zeros(2 * n, dtype=torch.float64, device=dev)
    a = torch.zeros(n, dtype=torch.float64, device=dev)
    cd.linear_functional(fem, cd.GAUSSIANS, f[:n], param=omega)
    cd.linear_functional(fem, cd.ALPHA_DISK, a)
    cd.DiagInvMassMatrix(fem).action(a, a)
    Ws = {tag: cd.WaveHoltz(omega, a.cpu().numpy(), fem, integrator="rk4", coarsen=4, stiffness="lobatto", sweep="lattice", precision=tag) for tag in ("f64", "f32")}
    b64, y = torch.empty_like(f), torch.empty_like(f)
    Ws["f64"].rhs(f, b64)
    for tag, W in Ws.items():
        b, z = torch.empty_like(f), torch.zeros_like(f)
        W.rhs(f, b)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = cd.gmres(2 * n, z, W, b, 20, 400, 1e-4, max_seconds=300.0)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        Ws["f64"].action(z, y)
        true_res = float(torch.linalg.norm(b64 - y) / torch.linalg.norm(b64))
        info = W.info()
        say(f"lattice32 solve nx={nx} ndof={n} omega={omega:.2f} disk coefficient rk4/4 nt={info['nt']} GMRES(20) tol 1e-4 precision={tag} [{info['stiffness_kernel']}]: "
            f"success={out.success} matvecs={out.num_matvec} cycles={out.num_iter} rel_res={out.res_norm[-1] / out.res_norm[0]:.3e} "
            f"residual in the f64 operator={true_res:.3e} seconds={sec:.2f} ms_per_period={1e3 * sec / max(1, out.num_matvec):.2f} "
            f"us_per_sweep={1e6 * sec / max(1, out.num_matvec) / info['sweeps_per_period']:.1f} finite={bool(torch.isfinite(z).all())}")


PAIR_VECTORS = {"rk2": (18, 10), "rk4": (46, 22)}  # per lattice slot and time step: per-sweep, paired


def pair_step(nx):
    L, st = N.lib, stream()
    dt = 1e-9  # (the timed launches repeat on the same vectors: keep them bounded)
    fs, slots, keep = {}, {}, []
    for tag, dtype, multiple in (("f64", torch.float64, 2), ("f32", torch.float32, 4)):
        D, Lx = lattice_description(nx, multiple)
        m = D.stride * Lx
        slots[tag] = m
        g = torch.Generator(device=dev).manual_seed(1)
        v = {k: torch.randn(m, dtype=dtype, device=dev, generator=g) for k in ("p", "q", "u", "v", "ps", "ps2", "qs", "aq", "ap")}
        v["invm"] = torch.rand(m, dtype=dtype, device=dev, generator=g) + 0.5
        v["Hi"] = torch.zeros(m, dtype=dtype, device=dev)
        if D.stride > Lx:  # the padding columns: zero state, invm = 0
            for t in v.values():
                t.view(Lx, D.stride)[:, Lx:] = 0.0
        a, d = {k: p(t) for k, t in v.items()}, C.byref(D)
        keep.append((D, v))
        one = (lambda name: getattr(L, f"cuddh_hip_wave_lattice_{name}_f64")) if tag == "f64" else (lambda name: getattr(L, f"cuddh_hip_wave32_{name}"))
        two = (lambda name: getattr(L, f"cuddh_hip_wave_pair_{name}_f64")) if tag == "f64" else (lambda name: getattr(L, f"cuddh_hip_wave_pair32_{name}"))

        def sweep_rk2(a=a, d=d, one=one):
            N.check(one("rk2_a")(d, dt / 2, 1.0, 0.0, a["p"], a["q"], a["invm"], a["Hi"], None, None, a["qs"], a["ps"], st))
            N.check(one("rk2_b")(d, dt, 1.0, 0.0, 1e-3, a["ps"], a["qs"], a["invm"], a["Hi"], None, None, a["p"], a["q"], a["u"], a["v"], st))

        def sweep_rk4(a=a, d=d, one=one):
            N.check(one("rk4_1")(d, dt / 2, 1.0, 0.0, a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps"], a["qs"], a["aq"], a["ap"], st))
            N.check(one("rk4_2")(d, dt / 2, 1.0, 0.0, a["ps"], a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps2"], a["qs"], a["aq"], a["ap"], st))
            N.check(one("rk4_3")(d, dt, 1.0, 0.0, a["ps2"], a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps"], a["qs"], a["aq"], a["ap"], st))
            N.check(one("rk4_4")(d, dt / 6, 1.0, 0.0, 1e-3, a["ps"], a["qs"], a["aq"], a["ap"], a["invm"], a["Hi"], None, None, a["p"], a["q"], a["u"], a["v"], st))

        state2, state4 = {"P": ("p", "ps"), "Q": ("q", "qs")}, {"P": ("p", "ps")}

        def pair_rk2(a=a, d=d, two=two, s=state2):
            (P, P2), (Q, Q2) = s["P"], s["Q"]
            N.check(two("rk2")(d, dt / 2, dt, 1.0, 0.0, 1.0, 0.0, 1e-3, a[P], a[Q], a["invm"], a["Hi"], None, None, a[P2], a[Q2], a["u"], a["v"], st))
            s["P"], s["Q"] = (P2, P), (Q2, Q)

        def pair_rk4(a=a, d=d, two=two, s=state4):
            P, P2 = s["P"]
            N.check(two("rk4_12")(d, dt / 2, 1.0, 0.0, 1.0, 0.0, a[P], a["q"], a["invm"], a["Hi"], None, None, a["ps2"], a["qs"], a["aq"], a["ap"], st))
            N.check(two("rk4_34")(d, dt, dt / 6, 1.0, 0.0, 1.0, 0.0, 1e-3, a["ps2"], a[P], a["qs"], a["aq"], a["ap"], a["invm"], a["Hi"], None, None,
                                  a[P2], a["q"], a["u"], a["v"], st))
            s["P"] = (P2, P)

        fs.update({f"rk2 sweep {tag}": sweep_rk2, f"rk2 pair {tag}": pair_rk2, f"rk4 sweep {tag}": sweep_rk4, f"rk4 pair {tag}": pair_rk4})
    t = timed(fs, inner=20)
    say(f"pair step nx={nx} slots f64 {slots['f64']} ({8 * slots['f64'] / 1e6:.1f} MB per vector), f32 {slots['f32']} ({4 * slots['f32'] / 1e6:.1f} MB per vector); "
        f"pair tiles f64 {L.cuddh_hip_wave_pair_tile_x()} x {L.cuddh_hip_wave_pair_tile_y()}, f32 {L.cuddh_hip_wave_pair32_tile_x()} x {L.cuddh_hip_wave_pair32_tile_y()}")
    size = {"f64": 8, "f32": 4}
    for scheme in ("rk2", "rk4"):
        for tag in ("f64", "f32"):
            (ms, ls, hs), (mp, lp, hp) = t[f"{scheme} sweep {tag}"], t[f"{scheme} pair {tag}"]
            vs, vp = PAIR_VECTORS[scheme]
            rate = lambda vectors, ms_: vectors * size[tag] * slots[tag] / (ms_ * 1e-3) / 1e12  # noqa: E731
            say(f"  {scheme} {tag} us per time step: per-sweep {1e3 * ms:8.1f} (min {1e3 * ls:.1f} max {1e3 * hs:.1f}) {vs} vectors {rate(vs, ms):5.2f} TB/s;  "
                f"paired {1e3 * mp:8.1f} (min {1e3 * lp:.1f} max {1e3 * hp:.1f}) {vp} vectors {rate(vp, mp):5.2f} TB/s;  paired / per-sweep {mp / ms:.3f} "
                f"(byte model {vp / vs:.2f})")
    del keep


def pair_period(nx):
    mesh, fem = space(nx)
    n = fem.size()
    omega = 2 * math.pi * nx / 10
    g = torch.Generator(device=dev).manual_seed(2)
    z = torch.randn(2 * n, dtype=torch.float64, device=dev, generator=g)
    for scheme, coarsen in (("rk2", None), ("rk4", 4)):
        for tag in ("f64", "f32"):
            Ws = {launch: cd.WaveHoltz(omega, np.ones(n), fem, integrator=scheme, coarsen=coarsen, stiffness="lobatto", sweep="lattice", precision=tag,
                                       launch=launch) for launch in ("sweep", "pair")}
            out = {k: torch.empty_like(z) for k in Ws}
            for k, W in Ws.items():
                W.period(z, None, out[k])
            torch.cuda.synchronize()
            same = torch.equal(out["sweep"], out["pair"])
            info = Ws["pair"].info()
            t = timed({k: (lambda W=W, k=k: W.period(z, None, out[k])) for k, W in Ws.items()}, inner=1)
            text = "; ".join(f"{k} {t[k][0]:.2f} ms (min {t[k][1]:.2f} max {t[k][2]:.2f}) = {1e3 * t[k][0] / info['nt']:.1f} us per time step "
                             f"[{Ws[k].info()['stiffness_kernel']}]" for k in Ws)
            vs, vp = PAIR_VECTORS[scheme]
            say(f"pair period nx={nx} ndof={n} {scheme} {tag} nt={info['nt']}: {text}; paired / per-sweep {t['pair'][0] / t['sweep'][0]:.3f} "
                f"(byte model {vp / vs:.2f}); results bit-identical: {same}")
            del Ws, out


def pair_solve(nx):
    mesh, fem = space(nx)
    n = fem.size()
    omega = 2 * math.pi * nx / 10
    f = torch.zeros(2 * n, dtype=torch.float64, device=dev)
    a = torch.zeros(n, dtype=torch.float64, device=dev)
    cd.linear_functional(fem, cd.GAUSSIANS, f[:n], param=omega)
    cd.linear_functional(fem, cd.ALPHA_DISK, a)
    cd.DiagInvMassMatrix(fem).action(a, a)
    for tag in ("f64", "f32"):
        sec, sol = {}, {}
        for launch in ("sweep", "pair"):
            W = cd.WaveHoltz(omega, a.cpu().numpy(), fem, integrator="rk4", coarsen=4, stiffness="lobatto", sweep="lattice", precision=tag, launch=launch)
            b, z = torch.empty_like(f), torch.zeros_like(f)
            W.rhs(f, b)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = cd.gmres(2 * n, z, W, b, 20, 400, 1e-4, max_seconds=300.0)
            torch.cuda.synchronize()
            sec[launch], sol[launch] = time.perf_counter() - t0, z
            info = W.info()
            say(f"pair solve nx={nx} ndof={n} omega={omega:.2f} disk coefficient rk4/4 nt={info['nt']} GMRES(20) tol 1e-4 precision={tag} launch={launch} "
                f"[{info['stiffness_kernel']}]: success={out.success} matvecs={out.num_matvec} cycles={out.num_iter} rel_res={out.res_norm[-1] / out.res_norm[0]:.3e} "
                f"seconds={sec[launch]:.2f} ms_per_period={1e3 * sec[launch] / max(1, out.num_matvec):.2f} finite={bool(torch.isfinite(z).all())}")
            del W
        say(f"pair solve nx={nx} {tag}: paired / per-sweep seconds {sec['pair'] / sec['sweep']:.3f}; solutions bit-identical: {torch.equal(sol['pair'], sol['sweep'])}")


def cells_step(nx):
    L, st = N.lib, stream()
    dt = 1e-9  # (the timed launches repeat on the same vectors: keep them bounded)
    fs, slots, keep = {}, {}, []
    full = torch.ones(nx * nx, dtype=torch.uint8, device=dev)
    quarter = full.clone()
    quarter.view(nx, nx)[nx // 2:, nx // 2:] = 0
    for tag, dtype, multiple in (("f64", torch.float64, 2), ("f32", torch.float32, 4)):
        D, Lx = lattice_description(nx, multiple)
        m = D.stride * Lx
        slots[tag] = m
        g = torch.Generator(device=dev).manual_seed(1)
        v = {k: torch.randn(m, dtype=dtype, device=dev, generator=g) for k in ("p", "q", "u", "v", "ps", "ps2", "qs", "aq", "ap")}
        v["invm"] = torch.rand(m, dtype=dtype, device=dev, generator=g) + 0.5
        v["Hi"] = torch.zeros(m, dtype=dtype, device=dev)
        if D.stride > Lx:  # the padding columns: zero state, invm = 0
            for t in v.values():
                t.view(Lx, D.stride)[:, Lx:] = 0.0
        a, d = {k: p(t) for k, t in v.items()}, C.byref(D)
        keep.append((D, v))
        lat = (lambda name: getattr(L, f"cuddh_hip_wave_lattice_{name}_f64")) if tag == "f64" else (lambda name: getattr(L, f"cuddh_hip_wave32_{name}"))
        cel = (lambda name: getattr(L, f"cuddh_hip_wave_cells_{name}_f64")) if tag == "f64" else (lambda name: getattr(L, f"cuddh_hip_wave_cells32_{name}"))

        def step(scheme, fn, head, a=a):
            if scheme == "rk2":
                N.check(fn("rk2_a")(*head, dt / 2, 1.0, 0.0, a["p"], a["q"], a["invm"], a["Hi"], None, None, a["qs"], a["ps"], st))
                N.check(fn("rk2_b")(*head, dt, 1.0, 0.0, 1e-3, a["ps"], a["qs"], a["invm"], a["Hi"], None, None, a["p"], a["q"], a["u"], a["v"], st))
            else:
                N.check(fn("rk4_1")(*head, dt / 2, 1.0, 0.0, a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps"], a["qs"], a["aq"], a["ap"], st))
                N.check(fn("rk4_2")(*head, dt / 2, 1.0, 0.0, a["ps"], a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps2"], a["qs"], a["aq"], a["ap"], st))
                N.check(fn("rk4_3")(*head, dt, 1.0, 0.0, a["ps2"], a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps"], a["qs"], a["aq"], a["ap"], st))
                N.check(fn("rk4_4")(*head, dt / 6, 1.0, 0.0, 1e-3, a["ps"], a["qs"], a["aq"], a["ap"], a["invm"], a["Hi"], None, None, a["p"], a["q"], a["u"], a["v"], st))

        for scheme in ("rk2", "rk4"):
            fs[f"{scheme} lattice {tag}"] = lambda scheme=scheme, lat=lat, d=d, step=step: step(scheme, lat, (d,))
            fs[f"{scheme} cells {tag}"] = lambda scheme=scheme, cel=cel, d=d, step=step: step(scheme, cel, (d, p(full)))
            fs[f"{scheme} quarter {tag}"] = lambda scheme=scheme, cel=cel, d=d, step=step: step(scheme, cel, (d, p(quarter)))
    t = timed(fs, inner=20)
    say(f"cells step nx={nx} slots f64 {slots['f64']} ({8 * slots['f64'] / 1e6:.1f} MB per vector), f32 {slots['f32']} ({4 * slots['f32'] / 1e6:.1f} MB per vector); "
        f"tile {L.cuddh_hip_wave_lattice_tile_x()} x {L.cuddh_hip_wave_lattice_tile_y()}; us per time step, median of {reps} (min max)")
    for scheme in ("rk2", "rk4"):
        for tag in ("f64", "f32"):
            (ml, ll, hl), (mc, lc, hc), (mq, lq, hq) = (t[f"{scheme} {k} {tag}"] for k in ("lattice", "cells", "quarter"))
            say(f"  {scheme} {tag}: wave_lattice {1e3 * ml:8.1f} ({1e3 * ll:.1f} {1e3 * hl:.1f});  wave_cells, every cell present {1e3 * mc:8.1f} ({1e3 * lc:.1f} {1e3 * hc:.1f}), "
                f"cells / lattice {mc / ml:.3f};  a quadrant of cells removed {1e3 * mq:8.1f} ({1e3 * lq:.1f} {1e3 * hq:.1f}), quadrant / every cell {mq / mc:.3f} "
                f"(cells left: 0.75)")
    del keep


def cells_solve(nx):
    k0, k1 = 5 * nx // 8, 6 * nx // 8  # the obstacle: nx / 8 x nx / 8 cells at [0.25, 0.5]^2
    present = np.ones((nx, nx), dtype=bool)
    present[k0:k1, k0:k1] = False
    mesh = cd.Mesh2D.grid_cells(nx, -1.0, 1.0, nx, -1.0, 1.0, present)
    fem = cd.H1Space(mesh, cd.Basis(NB))
    n = fem.size()
    xy, edges, boundary = mesh.vertices(), mesh.edges(), mesh.boundary_edges()
    ends = np.stack([xy[edges[boundary, 1]], xy[edges[boundary, 2]]])  # (2, n_boundary, 2)
    outer = boundary[np.any(np.all(np.abs(np.abs(ends) - 1.0) < 1e-12, axis=0), axis=1)]  # both ends on x = +-1 or both on y = +-1
    omega = 2 * math.pi * nx / 10
    f = torch.zeros(2 * n, dtype=torch.float64, device=dev)
    a = torch.zeros(n, dtype=torch.float64, device=dev)
    cd.linear_functional(fem, cd.GAUSSIANS, f[:n], param=omega)
    cd.linear_functional(fem, cd.ALPHA_DISK, a)
    cd.DiagInvMassMatrix(fem).action(a, a)
    say(f"cells solve nx={nx}: {mesh.n_elem()} of {nx * nx} cells, ndof={n}, obstacle cells [{k0}, {k1})^2 sound-hard ({len(outer)} of {len(boundary)} boundary edges absorbing), "
        f"omega={omega:.2f}, disk coefficient, rk4/4, GMRES(20) tol 1e-4")
    sec = {}
    for name, kw in (("lattice f64", dict(sweep="lattice")), ("lattice f32", dict(sweep="lattice", precision="f32")), ("operator/lobatto", dict(sweep="operator"))):
        W = cd.WaveHoltz(omega, a.cpu().numpy(), fem, integrator="rk4", coarsen=4, stiffness="lobatto", faces=outer, **kw)
        b, z = torch.empty_like(f), torch.zeros_like(f)
        W.rhs(f, b)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = cd.gmres(2 * n, z, W, b, 20, 400, 1e-4, max_seconds=200.0)
        torch.cuda.synchronize()
        sec[name] = time.perf_counter() - t0
        info = W.info()
        say(f"  {name:16s} [{info['stiffness_kernel']}] nt={info['nt']}: success={out.success} matvecs={out.num_matvec} cycles={out.num_iter} "
            f"rel_res={out.res_norm[-1] / out.res_norm[0]:.3e} seconds={sec[name]:.2f} ms_per_period={1e3 * sec[name] / max(1, out.num_matvec):.2f} "
            f"us_per_sweep={1e6 * sec[name] / max(1, out.num_matvec) / info['sweeps_per_period']:.1f} finite={bool(torch.isfinite(z).all())}")
        del W
    say(f"  seconds: lattice f64 / operator {sec['lattice f64'] / sec['operator/lobatto']:.3f}, lattice f32 / operator {sec['lattice f32'] / sec['operator/lobatto']:.3f}")


def weights_step(nx):
    L, st = N.lib, stream()
    dt = 1e-9  # (the timed launches repeat on the same vectors: keep them bounded)
    fs, slots, keep = {}, {}, []
    flags = torch.ones(nx * nx, dtype=torch.uint8, device=dev)
    for tag, dtype, multiple in (("f64", torch.float64, 2), ("f32", torch.float32, 4)):
        D, Lx = lattice_description(nx, multiple)
        m = D.stride * Lx
        slots[tag] = m
        g = torch.Generator(device=dev).manual_seed(1)
        v = {k: torch.randn(m, dtype=dtype, device=dev, generator=g) for k in ("p", "q", "u", "v", "ps", "ps2", "qs", "aq", "ap")}
        v["invm"] = torch.rand(m, dtype=dtype, device=dev, generator=g) + 0.5
        v["Hi"] = torch.zeros(m, dtype=dtype, device=dev)
        if D.stride > Lx:  # the padding columns: zero state, invm = 0
            for t in v.values():
                t.view(Lx, D.stride)[:, Lx:] = 0.0
        ones = torch.ones(nx * nx, dtype=dtype, device=dev)
        a, d = {k: p(t) for k, t in v.items()}, C.byref(D)
        keep.append((D, v, ones))
        lat = (lambda name: getattr(L, f"cuddh_hip_wave_lattice_{name}_f64")) if tag == "f64" else (lambda name: getattr(L, f"cuddh_hip_wave32_{name}"))
        cel = (lambda name: getattr(L, f"cuddh_hip_wave_cells_{name}_f64")) if tag == "f64" else (lambda name: getattr(L, f"cuddh_hip_wave_cells32_{name}"))
        wts = (lambda name: getattr(L, f"cuddh_hip_wave_weights_{name}_f64")) if tag == "f64" else (lambda name: getattr(L, f"cuddh_hip_wave_weights32_{name}"))

        def step(scheme, fn, head, a=a):
            if scheme == "rk2":
                N.check(fn("rk2_a")(*head, dt / 2, 1.0, 0.0, a["p"], a["q"], a["invm"], a["Hi"], None, None, a["qs"], a["ps"], st))
                N.check(fn("rk2_b")(*head, dt, 1.0, 0.0, 1e-3, a["ps"], a["qs"], a["invm"], a["Hi"], None, None, a["p"], a["q"], a["u"], a["v"], st))
            else:
                N.check(fn("rk4_1")(*head, dt / 2, 1.0, 0.0, a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps"], a["qs"], a["aq"], a["ap"], st))
                N.check(fn("rk4_2")(*head, dt / 2, 1.0, 0.0, a["ps"], a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps2"], a["qs"], a["aq"], a["ap"], st))
                N.check(fn("rk4_3")(*head, dt, 1.0, 0.0, a["ps2"], a["p"], a["q"], a["invm"], a["Hi"], None, None, a["ps"], a["qs"], a["aq"], a["ap"], st))
                N.check(fn("rk4_4")(*head, dt / 6, 1.0, 0.0, 1e-3, a["ps"], a["qs"], a["aq"], a["ap"], a["invm"], a["Hi"], None, None, a["p"], a["q"], a["u"], a["v"], st))

        for scheme in ("rk2", "rk4"):
            fs[f"{scheme} lattice {tag}"] = lambda scheme=scheme, lat=lat, d=d, step=step: step(scheme, lat, (d,))
            fs[f"{scheme} cells {tag}"] = lambda scheme=scheme, cel=cel, d=d, step=step: step(scheme, cel, (d, p(flags)))
            fs[f"{scheme} weights {tag}"] = lambda scheme=scheme, wts=wts, d=d, step=step, ones=ones: step(scheme, wts, (d, p(ones)))
    t = timed(fs, inner=20)
    say(f"weights step nx={nx} slots f64 {slots['f64']} ({8 * slots['f64'] / 1e6:.1f} MB per vector), f32 {slots['f32']} ({4 * slots['f32'] / 1e6:.1f} MB per vector); "
        f"tile {L.cuddh_hip_wave_lattice_tile_x()} x {L.cuddh_hip_wave_lattice_tile_y()}; every weight and every flag 1; us per time step, median of {reps} (min max)")
    for scheme in ("rk2", "rk4"):
        for tag in ("f64", "f32"):
            (ml, ll, hl), (mc, lc, hc), (mw, lw, hw) = (t[f"{scheme} {k} {tag}"] for k in ("lattice", "cells", "weights"))
            say(f"  {scheme} {tag}: wave_lattice {1e3 * ml:8.1f} ({1e3 * ll:.1f} {1e3 * hl:.1f});  wave_cells {1e3 * mc:8.1f} ({1e3 * lc:.1f} {1e3 * hc:.1f});  "
                f"wave_weights {1e3 * mw:8.1f} ({1e3 * lw:.1f} {1e3 * hw:.1f});  weights / cells {mw / mc:.3f}, weights / lattice {mw / ml:.3f}")
    del keep


def weights_solve(nx):
    k0, k1 = 5 * nx // 8, 6 * nx // 8  # the inclusion: nx / 8 x nx / 8 cells at [0.25, 0.5]^2
    beta = np.ones((nx, nx))
    beta[k0:k1, k0:k1] = 4.0
    mesh, fem = space(nx)
    n = fem.size()
    omega = 2 * math.pi * nx / 10
    f = torch.zeros(2 * n, dtype=torch.float64, device=dev)
    a = torch.zeros(n, dtype=torch.float64, device=dev)
    cd.linear_functional(fem, cd.GAUSSIANS, f[:n], param=omega)
    cd.linear_functional(fem, cd.ALPHA_DISK, a)
    cd.DiagInvMassMatrix(fem).action(a, a)
    say(f"weights solve nx={nx}: ndof={n}, beta = 4 on the cells [{k0}, {k1})^2 and 1 elsewhere, omega={omega:.2f}, disk coefficient, rk4/4, "
        f"every boundary edge absorbing, GMRES(20) tol 1e-4")
    sec = {}
    for name, kw in (("weights f64", dict(cell_stiffness=beta.reshape(-1))), ("weights f32", dict(cell_stiffness=beta.reshape(-1), precision="f32")),
                     ("beta = 1 f64", dict()), ("beta = 1 f32", dict(precision="f32"))):
        W = cd.WaveHoltz(omega, a.cpu().numpy(), fem, integrator="rk4", coarsen=4, stiffness="lobatto", sweep="lattice", **kw)
        b, z = torch.empty_like(f), torch.zeros_like(f)
        W.rhs(f, b)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = cd.gmres(2 * n, z, W, b, 20, 400, 1e-4, max_seconds=200.0)
        torch.cuda.synchronize()
        sec[name] = time.perf_counter() - t0
        info = W.info()
        say(f"  {name:14s} [{info['stiffness_kernel']}] nt={info['nt']}: success={out.success} matvecs={out.num_matvec} cycles={out.num_iter} "
            f"rel_res={out.res_norm[-1] / out.res_norm[0]:.3e} seconds={sec[name]:.2f} ms_per_period={1e3 * sec[name] / max(1, out.num_matvec):.2f} "
            f"us_per_sweep={1e6 * sec[name] / max(1, out.num_matvec) / info['sweeps_per_period']:.1f} finite={bool(torch.isfinite(z).all())}")
        del W


say(f"waveholtz_rates: {torch.cuda.get_device_name(0)}, n_basis {NB}, a == 1, omega = 2 pi nx / 10, reps {reps}")
for part, fn, ns in (("stages", stages, sizes), ("period", period, sizes), ("solve", solve, solve_sizes), ("lattice_stages", lattice_stages, sizes),
                     ("lattice_period", lattice_period, sizes), ("lattice_solve", lattice_solve, solve_sizes),
                     ("lattice32_stages", lattice32_stages, sizes), ("lattice32_period", lattice32_period, sizes),
                     ("lattice32_solve", lattice32_solve, solve_sizes), ("pair_step", pair_step, sizes), ("pair_period", pair_period, sizes),
                     ("pair_solve", pair_solve, solve_sizes), ("cells_step", cells_step, sizes), ("cells_solve", cells_solve, solve_sizes),
                     ("weights_step", weights_step, sizes), ("weights_solve", weights_solve, solve_sizes)):
    if part in parts:
        for nx in ns:
            fn(nx)
