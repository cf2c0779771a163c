"""DDH kernel 8: the dense 16x16 element matrix of kernel 5 applied on the fp64 matrix cores (v_mfma_f64_16x16x4_f64).

Kernel 8 is the fp64 (parity) mode's counterpart of the benchmarked fp32 kernel 5.  It computes the same local solves as the
sum-factorised fp64 kernels 1 and 2 with the element matrix formed and kept in double, so it is held to their gates: 1e-10
against the fp64 oracle, bitwise reproducibility of every entry point, and the physics check of tests/test_ddh_physics.py.
It is selected on request only (auto keeps fp64 on kernel 3); every distance is printed (`pytest -s`).
"""
import math
import time

import numpy as np
import pytest

import oracle
from conftest import GOLDEN
from test_baseline_regime import CONFIGS, Window
from test_ddh_physics import Case
from test_ddh_physics import product as physics_product
from test_gpu_parity import ddh_case, rel, to_dev

pytestmark = pytest.mark.gpu


def make(nx, nb, precision, kernel, h_a=None, omega=None, mesh=None):
    import cuddhelmholtz_amd as cd

    mesh = mesh or cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0)
    fem = cd.H1Space(mesh, cd.Basis(nb))
    if omega is None:
        omega = 2 * math.pi * nx / 10
    if h_a is None:
        h_a = np.ones(fem.size())
    F = cd.DDH(omega, h_a, fem, nx, nx, precision=precision, kernel=kernel)
    F._keep = (mesh, fem)
    return F


# ------------------------------------------------------------------ selection and rejection
@pytest.mark.parametrize("nx", [8, 16, 32])
def test_kernel8_selected_in_fp64(cuda, nx):
    F = make(nx, 4, "f64", 8)
    info = F.info()
    assert info["kernel"] == 8 and info["is_f64"] == 1


@pytest.mark.parametrize("nx,nb,precision,kernel", [(8, 4, "f32", 8), (10, 3, "f64", 8), (9, 5, "f64", 8), (8, 8, "f64", 8),
                                                    (8, 4, "f64", 5)])
def test_kernel8_rejected_where_it_does_not_apply(cuda, nx, nb, precision, kernel):
    """fp32, n_basis other than 4, and kernel 5 in fp64 (unchanged): an explicit request that does not apply is an error"""
    F = make(nx, nb, precision, kernel)
    with pytest.raises(RuntimeError):
        F.info()


def test_auto_still_picks_kernel3_in_fp64(cuda):
    assert make(8, 4, "f64", 0).info()["kernel"] == 3
    assert make(8, 4, "f32", 0).info()["kernel"] == 5


def test_kernel8_rejected_on_nonuniform_metric(cuda):
    """rectangles of varying width (x stretched smoothly, same element numbering as uniform_rect): kernel 2 runs, kernel 8 needs one
    metric tensor for all elements and refuses.  What kernel 2 computes there (g00 and g11 varying from element to element) is
    compared with the oracle on the same vertices at the fp64 gate."""
    import torch

    import cuddhelmholtz_amd as cd

    nx = 8
    base = cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0)
    xy = base.vertices().copy()
    xy[:, 0] = xy[:, 0] + 0.1 * np.sin(math.pi * xy[:, 0])  # monotone, keeps x = +-1
    mesh = cd.Mesh2D.from_vertices(xy, base.elements())
    assert make(nx, 4, "f64", 2, mesh=mesh).info()["kernel"] == 2
    F = make(nx, 4, "f64", 8, mesh=mesh)
    with pytest.raises(RuntimeError):
        F.info()

    omega = 2 * math.pi * nx / 10
    d = oracle.Discretization(oracle.Mesh(xy, base.elements()), 4)
    h_a = d.nodal(oracle.alpha_disk)
    fh = np.concatenate([oracle.linear_functional(d, oracle.gaussians(omega)), 0.1 * oracle.linear_functional(d, oracle.mass_poly)])
    O = oracle.DDH(d, nx, nx, omega, h_a, np.float64)
    per_element = np.round(O.G[0].reshape(16, -1, order="F"), 12)
    assert np.unique(per_element, axis=1).shape[1] == nx // 2 and not O.G[1].any()  # one metric per element width, all diagonal
    F = make(nx, 4, "f64", 2, h_a=h_a, omega=omega, mesh=mesh)
    assert F.info()["kernel"] == 2 and F.info()["nt"] == O.t.nt and F.size() == O.size
    n = F.size()
    lam_h = np.random.default_rng(2).standard_normal(n)
    used = np.unique(O.t.B[O.t.B >= 0])
    lam_h[np.setdiff1d(np.arange(n), np.concatenate([used, used + O.t.n_lambda]))] = 0.0
    written = np.unique(O.t.B[:, 1, :][O.t.B[:, 1, :] >= 0])
    written = np.concatenate([written, written + O.t.n_lambda])
    f, lam = to_dev(torch, fh, cuda), to_dev(torch, lam_h, cuda)
    b = torch.zeros(n, dtype=torch.float64, device=cuda)
    F.rhs(f, b)
    y = torch.full((n,), 5.0, dtype=torch.float64, device=cuda)
    F.action(lam, y)
    u = torch.full((2 * d.ndof,), 9.0, dtype=torch.float64, device=cuda)
    F.postprocess(lam, f, u)
    e = (rel(b.cpu().numpy(), O.rhs(fh)), rel(y.cpu().numpy()[written], O.action(lam_h)[written]), rel(u.cpu().numpy(), O.postprocess(lam_h, fh)))
    print(f"DDH64 kernel 2 on stretched rectangles vs fp64 oracle: rhs {e[0]:.2e} action {e[1]:.2e} postprocess {e[2]:.2e}")
    assert max(e) <= 1e-10, e


# ------------------------------------------------------------------ entry points vs the fp64 oracle
@pytest.mark.parametrize("nx", [8, 16])
def test_kernel8_entry_points(cuda, nx):
    """the case of test_gpu_parity.test_ddh_fp64_entry_points (example regime, disk coefficient)"""
    import torch

    import cuddhelmholtz_amd as cd

    nb = 4
    omega, d, h_a, fh = ddh_case(nx, nb)
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), cd.Basis(nb))
    F = cd.DDH(omega, h_a, fem, nx, nx, precision="f64", kernel=8)
    O = oracle.DDH(d, nx, nx, omega, h_a, np.float64)
    assert F.info()["kernel"] == 8
    f = to_dev(torch, fh, cuda)
    n = F.size()
    b = torch.zeros(n, dtype=torch.float64, device=cuda)
    F.rhs(f, b)
    e_b = rel(b.cpu().numpy(), O.rhs(fh))
    rng = np.random.default_rng(2)
    lam_h = rng.standard_normal(n)
    used = np.unique(O.t.B[O.t.B >= 0])
    lam_h[np.setdiff1d(np.arange(n), np.concatenate([used, used + O.t.n_lambda]))] = 0.0
    lam = to_dev(torch, lam_h, cuda)
    y = torch.full((n,), 5.0, dtype=torch.float64, device=cuda)
    F.action(lam, y)
    written = np.unique(O.t.B[:, 1, :][O.t.B[:, 1, :] >= 0])
    written = np.concatenate([written, written + O.t.n_lambda])
    e_y = rel(y.cpu().numpy()[written], O.action(lam_h)[written])
    u = torch.full((2 * d.ndof,), 9.0, dtype=torch.float64, device=cuda)
    F.postprocess(lam, f, u)
    e_u = rel(u.cpu().numpy(), O.postprocess(lam_h, fh))
    print(f"DDH64 kernel 8 {nx}x{nx} vs fp64 oracle: rhs {e_b:.2e} action {e_y:.2e} postprocess {e_u:.2e}")
    assert max(e_b, e_y, e_u) < 1e-10

    u2 = torch.full_like(u, -3.0)
    F.postprocess(lam, f, u2)
    assert torch.equal(u, u2)
    nd = F.info()["n_domains"]
    u3 = torch.full_like(u, 7.0)
    F.local_solution(0, nd // 2, lam, f, u3, True)
    F.local_solution(nd // 2, nd, lam, f, u3, False)
    assert torch.equal(u, u3)

    full = torch.zeros(n, dtype=torch.float64, device=cuda)
    F.local_traces(0, nd, f, lam, full)
    halves = torch.zeros_like(full)
    F.local_traces(0, nd // 2, f, lam, halves)
    F.local_traces(nd // 2, nd, f, lam, halves)
    assert torch.equal(halves, full)
    # listed launches (any order, odd counts) and the multi-GPU issue priority change nothing
    perm = np.random.default_rng(nx).permutation(nd).astype(np.int32)
    cut = max(1, nd // 3) | 1
    listed = torch.zeros_like(full)
    for ids in (perm[:cut], perm[cut:]):
        if len(ids):
            F.local_traces_listed(to_dev(torch, ids, cuda), f, lam, listed)
    assert torch.equal(listed, full)
    F.set_wave_priority(True)
    hi = torch.zeros_like(full)
    F.local_traces(0, nd, f, lam, hi)
    F.set_wave_priority(False)
    assert torch.equal(hi, full)
    # against kernel 2 (sum-factorised): the summation order alone differs
    F2 = cd.DDH(omega, h_a, fem, nx, nx, precision="f64", kernel=2)
    t2 = torch.zeros_like(full)
    F2.local_traces(0, nd, f, lam, t2)
    e_2 = rel(full.cpu().numpy(), t2.cpu().numpy())
    print(f"DDH64 kernel 8 vs kernel 2 local traces {nx}x{nx}: {e_2:.2e}")
    assert e_2 < 1e-11


def test_kernel8_matches_golden(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    G = np.load(GOLDEN / "hotpath_vectors.npz")
    tag = "ddh_8_4"
    nx, nb = int(G[f"{tag}_meta"][0]), int(G[f"{tag}_meta"][1])
    omega = float(G[f"{tag}_omega_dt"][0])
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), cd.Basis(nb))
    F = cd.DDH(omega, G[f"{tag}_h_a"], fem, nx, nx, precision="f64", kernel=8)
    info = F.info()
    assert info["kernel"] == 8
    assert (info["n_domains"], info["n_lambda"], info["nt"]) == tuple(int(v) for v in G[f"{tag}_meta"][2:])
    f = torch.from_numpy(G[f"{tag}_f"]).to(cuda)
    b = torch.zeros(F.size(), dtype=torch.float64, device=cuda)
    F.rhs(f, b)
    bg = torch.from_numpy(G[f"{tag}_b"]).to(cuda)
    Tb = torch.zeros_like(b)
    F.local_traces(0, info["n_domains"], None, bg, Tb)
    u = torch.zeros(2 * fem.size(), dtype=torch.float64, device=cuda)
    F.postprocess(bg, f, u)
    e = (rel(b.cpu().numpy(), G[f"{tag}_b"]), rel(Tb.cpu().numpy(), G[f"{tag}_Tb"]), rel(u.cpu().numpy(), G[f"{tag}_u"]))
    print(f"golden {tag} kernel 8 f64: rhs {e[0]:.2e}, T b {e[1]:.2e}, postprocess {e[2]:.2e}")
    assert max(e) < 1e-10


# ------------------------------------------------------------------ BASELINE's own regime (nt = 5120)
@pytest.mark.parametrize("coef", ["one", "disk"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_kernel8_window_parity(cuda, config, coef):
    """the windows of test_baseline_regime.test_ddh_window_parity, same gates: 1e-10 with a = 1, and with the disk coefficient
    (unstable local solves) 20 x the fp64 oracle's own sensitivity to inputs one ulp away"""
    import torch

    import cuddhelmholtz_amd as cd

    w = Window(config, coef)
    O64 = w.oracle_ddh(np.float64)
    assert (O64.t.nt, O64.t.n_domains) == (5120, 16)
    lam_h = w.traces(O64)
    written = w.written(O64)
    b64 = O64.rhs(w.f)
    y64 = O64.action(lam_h)
    u64 = O64.postprocess(lam_h, w.f)
    if coef == "one":
        gate = (1e-10, 1e-10, 1e-10)
    else:
        rng = np.random.default_rng(11)
        ulp = 2.0 ** -52
        f_p = w.f * (1 + ulp * rng.choice([-1.0, 1.0], w.f.size))
        lam_p = lam_h * (1 + ulp * rng.choice([-1.0, 1.0], lam_h.size))
        cond = (rel(O64.rhs(f_p), b64), rel(O64.action(lam_p)[written], y64[written]), rel(O64.postprocess(lam_p, f_p), u64))
        gate = tuple(max(1e-10, 20 * c) for c in cond)
        print(f"\n[{config}, a={coef}] fp64 oracle vs itself one ulp away: rhs {cond[0]:.2e} action {cond[1]:.2e} postprocess {cond[2]:.2e}")
    F, fem = w.product(cd, "f64", 8)
    assert F.info()["nt"] == 5120 and F.size() == O64.size
    n = F.size()
    f = torch.from_numpy(w.f).to(cuda)
    b = torch.zeros(n, dtype=torch.float64, device=cuda)
    F.rhs(f, b)
    lam = torch.from_numpy(lam_h).to(cuda)
    y = torch.zeros(n, dtype=torch.float64, device=cuda)
    F.action(lam, y)
    u = torch.zeros(2 * w.ndof, dtype=torch.float64, device=cuda)
    F.postprocess(lam, f, u)
    e = (rel(b.cpu().numpy(), b64), rel(y.cpu().numpy()[written], y64[written]), rel(u.cpu().numpy(), u64))
    print(f"[{config}, a={coef}] fp64 kernel 8 vs fp64 oracle: rhs {e[0]:.2e} action {e[1]:.2e} postprocess {e[2]:.2e} "
          f"(gates {gate[0]:.1e} {gate[1]:.1e} {gate[2]:.1e})")
    assert all(x < g for x, g in zip(e, gate)), (e, gate)


# ------------------------------------------------------------------ solve
@pytest.mark.parametrize("nx", [8, 32])
def test_kernel8_gmres_solve(cuda, nx):
    """rhs -> gmres(20, 20, 1e-10) -> postprocess with kernels 8 and 2: same matvec count, residual histories equal to 1e-10 of the
    initial residual, solutions within 1e-8 of each other; at 8^2 also within 1e-8 of the same flow on the fp64 oracle.
    At 8^2 the solve stalls above 1e-10 and runs all 400 matvecs, and two fp64 evaluation orders drift apart by ~1e-10 over them
    (measured 1.6e-10).  So that history gate is max(1e-10, 20 x the oracle's own sensitivity), as in
    test_baseline_regime.test_ddh_window_parity: the distance between two oracle runs whose right-hand sides are one ulp apart."""
    import torch

    import cuddhelmholtz_amd as cd

    nb = 4
    omega, d, h_a, fh = ddh_case(nx, nb)
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), cd.Basis(nb))
    f = to_dev(torch, fh, cuda)
    runs = {}
    for kernel in (8, 2):
        F = cd.DDH(omega, h_a, fem, nx, nx, precision="f64", kernel=kernel)
        assert F.info()["kernel"] == kernel
        n = F.size()
        b = torch.zeros(n, dtype=torch.float64, device=cuda)
        lam = torch.zeros_like(b)
        u = torch.zeros(2 * d.ndof, dtype=torch.float64, device=cuda)
        F.rhs(f, b)
        out = cd.gmres(n, lam, F, b, 20, 20, 1e-10)
        F.postprocess(lam, f, u)
        runs[kernel] = (out, u.cpu().numpy())
    (o8, u8), (o2, u2) = runs[8], runs[2]
    r8, r2 = np.asarray(o8.res_norm), np.asarray(o2.res_norm)
    assert len(r8) == len(r2)
    dr = float(np.max(np.abs(r8 - r2)) / r2[0])
    msg = (f"DDH64 solve {nx}x{nx}: kernel 8 {o8.num_matvec} matvecs (success {o8.success}), kernel 2 {o2.num_matvec}; "
           f"residual histories {dr:.2e}; u kernel 8 vs kernel 2 {rel(u8, u2):.2e}")
    gate = 1e-10
    if nx == 8:
        O = oracle.DDH(d, nx, nx, omega, h_a, np.float64)
        b_ref = O.rhs(fh)
        lam_ref, info = oracle.gmres(O.action, b_ref, m=20, maxit=20, tol=1e-10)
        u_ref = O.postprocess(lam_ref, fh)
        b_p = b_ref * (1 + 2.0 ** -52 * np.random.default_rng(11).choice([-1.0, 1.0], b_ref.size))
        _, info_p = oracle.gmres(O.action, b_p, m=20, maxit=20, tol=1e-10)
        ro, rp = np.asarray(info["res_norm"]), np.asarray(info_p["res_norm"])
        cond = float(np.max(np.abs(rp - ro)) / ro[0]) if len(rp) == len(ro) else 1.0
        gate = max(gate, 20 * cond)
        msg += (f"; oracle {info['num_matvec']} matvecs, u kernel 8 vs oracle {rel(u8, u_ref):.2e}; oracle history vs itself one ulp "
                f"away {cond:.2e} -> history gate {gate:.1e}")
        assert o8.success == info["success"] and abs(o8.num_matvec - info["num_matvec"]) <= 1
        assert rel(u8, u_ref) < 1e-8
    print(msg)
    assert o8.num_matvec == o2.num_matvec
    assert dr < gate
    assert rel(u8, u2) < 1e-8


# ------------------------------------------------------------------ physics
def test_kernel8_local_solves_vs_continuous_waveholtz(cuda):
    """tests/test_ddh_physics.py's check of the local solves against the WaveHoltz ODE, at its fp64 tolerance"""
    import torch

    c = Case(8, 8)
    F = physics_product(c, "f64", 8)
    assert F.info()["kernel"] == 8
    u = torch.zeros(2 * c.ndof, dtype=torch.float64, device=cuda)
    F.postprocess(torch.zeros(F.size(), dtype=torch.float64, device=cuda), torch.from_numpy(c.f).to(cuda), u)
    e = rel(u.cpu().numpy(), c.continuous_local_solves())
    print(f"product f64 kernel 8 local solves vs continuous WaveHoltz (8x8): {e:.2e}")
    assert e < 2e-4


# ------------------------------------------------------------------ speed floor
def test_kernel8_faster_than_kernel2(cuda):
    """loose floor against a silently slow path (the measured rates are in profiles/r04/ddh64_rates.txt): at 256^2, in one
    process, warm, best of 3, kernel 8's action takes at most 1 / 1.2 of kernel 2's"""
    import torch

    nx = 256
    best = {}
    for kernel in (2, 8):
        F = make(nx, 4, "f64", kernel, omega=math.pi * nx / 32)
        assert F.info()["kernel"] == kernel
        lam = torch.rand(F.size(), dtype=torch.float64, device=cuda)
        out = torch.zeros_like(lam)
        F.action(lam, out)
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            F.action(lam, out)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        best[kernel] = min(ts)
        del F
    print(f"DDH64 action 256^2: kernel 2 {best[2] * 1e3:.1f} ms, kernel 8 {best[8] * 1e3:.1f} ms ({best[2] / best[8]:.2f}x)")
    assert best[2] >= 1.2 * best[8]
