"""DDH.from_labels(integrator=, coarsen=, time_ratios=) on the device: kernels 9 (one wavefront per subdomain) and 10 (one
workgroup per subdomain) with per-subdomain time grids and RK4.

The case is tests/ddh_labels_rk.py: the reference's unstructured square (119 quads, not refined), n_basis 4, omega = 2 pi,
9 subdomains of 5 to 16 elements from Morton labels, a = 0.4 / 0.5 / 1, `coefficient` ratios 1, 2 and 3 (three step counts in
kernel 9's workgroups of four wavefronts).  References are computed once per session and shared.

  * parity of rhs / action (written slots) / postprocess, kernels 9 and 10, fp64 and fp32: RK2 with time_ratios="coefficient"
    against the per-subdomain oracle, RK4 / coarsen 4 on one grid and with "coefficient" against the numpy restatement
    (tests/ddh_rk.Restatement, pinned to the oracle on these labels in tests/test_ddh_labels_rk4.py).  fp64 at 1e-10, the
    project's gate; fp32 at 4 x the distance of the float32 reference to the float64 one, computed here (the floor rule of
    tests/test_gpu_ddh_block_size.py).  In fp32 the grids move the result by less than that floor, so time_ratios() is
    asserted and the fp64 case is what proves that the ratios were honoured;
  * block labels on the sweep case of tests/test_gpu_ddh_rk4.py against the cached reference the block kernels are held to;
  * kernel 10 off n_basis 4 (n_basis 5, 3 x 3-element blocks, 225 element nodes);
  * bitwise: integrator="rk2" and all-ones ratios against the plain plan, the full launch against ranges plus scrambled lists,
    two runs;
  * physics: rhs -> GMRES -> postprocess against ddh_general.fixed_point.
Every distance is printed (`pytest -s`).
"""
import math

import numpy as np
import pytest

import ddh_general as dg
import ddh_labels_rk as lr
import ddh_rk as rk
import oracle
from test_gpu_ddh_time_grids import RATIOS, block_labels, entry_points
from test_gpu_parity import rel, to_dev

pytestmark = pytest.mark.gpu

NAMES = ("rhs", "action", "postprocess")
FP64_GATE = 1e-10
COARSEN = lr.COARSEN
# distance of the restatement's own flow (rk4, coarsen 4, `coefficient` ratios, 12 WaveHoltz iterations, GMRES(100) to 1e-6) to
# ddh_general.fixed_point on tests/ddh_labels_rk.case, measured once on the CPU with
#   python profiles/tools/ddh_labels_rk4_restatement_flow.py 12 4 1e-10 1e-6        (239 matvecs; to 1e-10: 477 matvecs, 1.7312e-04:
# what is left is the time grid's error, not GMRES's, so the test stops at 1e-6; profiles/r14/README.md has the printed lines)
RESTATEMENT_FLOW_TO_FIXED_POINT = 1.7310e-04

# (id, keywords of from_labels, reference)
MODES = {
    "rk2-coefficient": (dict(time_ratios="coefficient"), lambda prec: lr.oracle_outputs(prec)),
    "rk4-one-grid": (dict(integrator="rk4", coarsen=COARSEN), lambda prec: lr.restated_outputs("rk4", COARSEN, False, prec)),
    "rk4-coefficient": (dict(integrator="rk4", coarsen=COARSEN, time_ratios="coefficient"), lambda prec: lr.restated_outputs("rk4", COARSEN, True, prec)),
}


def product_outputs(torch, cuda, F, c, f=None):
    b, y, u = (t.cpu().numpy().astype(np.float64) for t in entry_points(torch, cuda, F, c.f if f is None else f, c.lam, c.d.ndof))
    return b, y[c.written], u


def check_plan(F, c, kernel, mode):
    kw = MODES[mode][0]
    assert F.info()["kernel"] == kernel and F.size() == c.size
    assert F.integrator() == (kw.get("integrator", "rk2"), kw.get("coarsen", 1))
    assert F.info()["nt"] == rk.base_steps(c.nt_mesh, kw.get("coarsen", 1))
    assert list(F.time_ratios()) == (list(c.ratios) if "time_ratios" in kw else [1] * c.n_domains)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kernel", [9, 10])
def test_fp64_parity(cuda, kernel, mode):
    import torch

    c = lr.case()
    ref = MODES[mode][1]("f64")
    F = c.product("f64", kernel, **MODES[mode][0])
    check_plan(F, c, kernel, mode)
    e = [rel(a, r) for a, r in zip(product_outputs(torch, cuda, F, c), ref)]
    for nm, x in zip(NAMES, e):
        print(f"[unstructured square, {mode}, f64 kernel {kernel}] {nm}: vs fp64 reference {x:.3e} (gate {FP64_GATE:.0e})")
    assert all(np.linalg.norm(r) > 0 for r in ref)
    assert all(x <= FP64_GATE for x in e), e


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kernel", [9, 10])
def test_fp32_parity(cuda, kernel, mode):
    import torch

    c = lr.case()
    ref = MODES[mode][1]("f64")
    floor = [rel(a, r) for a, r in zip(MODES[mode][1]("f32"), ref)]
    F = c.product("f32", kernel, **MODES[mode][0])
    check_plan(F, c, kernel, mode)
    e = [rel(a, r) for a, r in zip(product_outputs(torch, cuda, F, c), ref)]
    for nm, x, fl in zip(NAMES, e, floor):
        print(f"[unstructured square, {mode}, f32 kernel {kernel}] {nm}: floor (float32 reference vs float64) {fl:.3e}, gate 4 x; product vs float64 "
              f"reference {x:.3e} ({x / fl:.2f} x floor)")
    assert all(np.linalg.norm(r) > 0 for r in ref)
    for nm, x, fl in zip(NAMES, e, floor):
        assert x <= 4 * fl, (nm, x, 4 * fl)


@pytest.mark.parametrize("kernel", [9, 10])
def test_block_labels_are_on_the_block_kernels_yardstick(cuda, kernel):
    """the sweep case of tests/test_gpu_ddh_rk4.py with that file's RATIOS: the reference kernels 1 / 2 / 8 are held to"""
    import torch

    import cuddhelmholtz_amd as cd

    c = rk.sweep_case(4)
    ref = rk.sweep_outputs(4, "rk4", COARSEN, RATIOS[4], "f64")
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(rk.NX, -1.0, 1.0, rk.NX, -1.0, 1.0), cd.Basis(4))
    F = cd.DDH.from_labels(c.omega, c.h_a, fem, block_labels(rk.NX, rk.NX, 4), precision="f64", kernel=kernel, integrator="rk4", coarsen=COARSEN,
                           time_ratios=np.asarray(RATIOS[4], dtype=np.int32))
    assert F.info()["kernel"] == kernel and F.integrator() == ("rk4", COARSEN) and list(F.time_ratios()) == list(RATIOS[4])
    assert F.info()["nt"] == rk.base_steps(c.nt_mesh, COARSEN) and F.size() == c.size
    b, y, u = (t.cpu().numpy().astype(np.float64) for t in entry_points(torch, cuda, F, c.fh, c.lam, c.d.ndof))
    e = [rel(a, r) for a, r in zip((b, y[c.written], u), ref)]
    for nm, x in zip(NAMES, e):
        print(f"[16 x 16 block labels, rk4 coarsen {COARSEN}, ratios {list(RATIOS[4])}, f64 kernel {kernel}] {nm}: vs fp64 restatement {x:.3e} (gate {FP64_GATE:.0e})")
    assert all(np.linalg.norm(r) > 0 for r in ref)
    assert all(x <= FP64_GATE for x in e), e


def test_kernel10_off_n_basis_4(cuda):
    """n_basis 5, 6 x 6 elements in four blocks of 3 x 3: 225 element nodes per subdomain"""
    import torch

    import cuddhelmholtz_amd as cd

    nx, nb, ratios = 6, 5, [1, 2, 1, 3]
    omega = 2 * math.pi * nx / 10
    d = oracle.Discretization(oracle.Mesh.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), nb)
    labels = block_labels(nx, nx, 3)
    h_a = np.ones(d.ndof)
    O = dg.OracleDDH(d, 4, labels, omega, h_a, np.float64)
    fh = np.concatenate([oracle.linear_functional(d, oracle.gaussians(omega)), 0.1 * oracle.linear_functional(d, oracle.mass_poly)])
    lam = np.random.default_rng(5).standard_normal(O.size)
    used = np.unique(O.t.B[O.t.B >= 0])
    lam[np.setdiff1d(np.arange(O.size), np.concatenate([used, used + O.t.n_lambda]))] = 0.0
    written = np.unique(O.t.B[:, 1, :][O.t.B[:, 1, :] >= 0])
    written = np.concatenate([written, written + O.t.n_lambda])
    b, y, u = rk.Restatement(O, "rk4", ratios, COARSEN).outputs(fh, lam)
    ref = (b, y[written], u)
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), cd.Basis(nb))
    F = cd.DDH.from_labels(omega, h_a, fem, labels, precision="f64", integrator="rk4", coarsen=COARSEN, time_ratios=np.asarray(ratios, dtype=np.int32))
    assert F.info()["kernel"] == 10 and F.info()["n_domains"] == 4 and F.info()["mx_dof"] <= 225 and list(F.time_ratios()) == ratios
    assert F.info()["nt"] == rk.base_steps(O.t.nt, COARSEN) and F.size() == O.size
    b, y, u = (t.cpu().numpy().astype(np.float64) for t in entry_points(torch, cuda, F, fh, lam, d.ndof))
    e = [rel(a, r) for a, r in zip((b, y[written], u), ref)]
    for nm, x in zip(NAMES, e):
        print(f"[6 x 6, n_basis 5, 3 x 3 block labels, rk4 coarsen {COARSEN}, ratios {ratios}, f64 kernel 10] {nm}: vs fp64 restatement {x:.3e} (gate {FP64_GATE:.0e})")
    assert all(np.linalg.norm(r) > 0 for r in ref)
    assert all(x <= FP64_GATE for x in e), e


@pytest.mark.parametrize("precision,kernel", [("f64", 9), ("f32", 9), ("f32", 10)])
def test_rk2_and_all_ones_ratios_are_bitwise_the_plain_plan(cuda, precision, kernel):
    """a == 1 (on this case's coefficient the mesh grid is outside RK2's stable range, and the plain plan is what is compared)"""
    import torch

    c = lr.case()
    F0 = c.product(precision, kernel, h_a=c.ones)
    F1 = c.product(precision, kernel, h_a=c.ones, integrator="rk2", coarsen=None, time_ratios=None)
    F2 = c.product(precision, kernel, h_a=c.ones, time_ratios=np.ones(c.n_domains, dtype=np.int32))  # per-subdomain path, one grid
    F4 = c.product(precision, kernel, h_a=c.ones, integrator="rk4", coarsen=1)
    assert F0.info() == F1.info() == F2.info() == F4.info() and F0.info()["kernel"] == kernel
    assert F1.integrator() == F2.integrator() == ("rk2", 1) and list(F2.time_ratios()) == [1] * c.n_domains
    out0, out1, out2, out4 = (entry_points(torch, cuda, F, c.f, c.lam, c.d.ndof) for F in (F0, F1, F2, F4))
    again = entry_points(torch, cuda, F2, c.f, c.lam, c.d.ndof)
    for nm, a, b1, b2, d, r in zip(NAMES, out0, out1, out2, out4, again):
        assert a.abs().max().item() > 0 and torch.isfinite(a).all()
        assert torch.equal(a, b1), nm
        assert torch.equal(a, b2), nm
        assert torch.equal(b2, r), nm
        assert not torch.equal(a, d), nm  # the scheme was honoured: on the same grid RK4 is another march


@pytest.mark.parametrize("precision,kernel", [("f64", 9), ("f32", 9), ("f32", 10)])
def test_launch_partitions_are_bitwise_the_full_launch(cuda, precision, kernel):
    import torch

    c = lr.case()
    F = c.product(precision, kernel, integrator="rk4", coarsen=COARSEN, time_ratios="coefficient")
    assert F.info()["kernel"] == kernel and list(F.time_ratios()) == list(c.ratios)
    nd = c.n_domains
    f = to_dev(torch, c.f, cuda)
    lam = to_dev(torch, c.lam.astype(np.float64 if F.f64 else np.float32), cuda)
    perm = np.random.default_rng(3).permutation(nd).astype(np.int32)
    for x, l in ((f, None), (None, lam), (f, lam)):
        full = torch.zeros(F.size(), dtype=F.trace_dtype, device=cuda)
        F.local_traces(0, nd, x, l, full)  # the plan's order: longest first
        assert full.abs().max().item() > 0
        twice = torch.zeros_like(full)
        F.local_traces(0, nd, x, l, twice)
        assert torch.equal(twice, full)
        ranged = torch.zeros_like(full)
        for d0, d1 in ((0, nd // 2 + 1), (nd // 2 + 1, nd)):
            F.local_traces(d0, d1, x, l, ranged)
        assert torch.equal(ranged, full)
        listed = torch.zeros_like(full)
        for ids in (perm[: nd // 3], perm[nd // 3:]):
            F.local_traces_listed(to_dev(torch, ids, cuda), x, l, listed)
        assert torch.equal(listed, full)


def _flow(torch, cuda, F, c, wh_iters):
    import cuddhelmholtz_amd as cd

    F.set_wh_iters(wh_iters)
    n = F.size()
    f = to_dev(torch, c.f, cuda)
    b = torch.zeros(n, dtype=F.trace_dtype, device=cuda)
    F.rhs(f, b)
    lam = torch.zeros_like(b)
    out = cd.gmres(n, lam, F, b, 100, 20, 1e-6)
    u = torch.zeros(2 * c.d.ndof, dtype=torch.float64, device=cuda)
    F.postprocess(lam, f, u)
    return u.cpu().numpy(), out


def test_physics_rk4_on_coefficient_grids_converges_to_the_exact_local_solve_fixed_point(cuda):
    import torch

    c = lr.case()
    O = c.O["f64"]
    want = dg.fixed_point(O.t, O.G, c.d.ndof, c.f)
    F = c.product("f64", 9, integrator="rk4", coarsen=COARSEN, time_ratios="coefficient")
    assert F.info()["kernel"] == 9 and list(F.time_ratios()) == list(c.ratios) and F.info()["nt"] == rk.base_steps(c.nt_mesh, COARSEN)
    u, out = _flow(torch, cuda, F, c, 12)
    e = rel(u, want)
    with np.errstate(all="ignore"):
        u0, out0 = _flow(torch, cuda, c.product("f64", 9), c, 12)
        e0 = rel(u0, want)
    gate = 2 * RESTATEMENT_FLOW_TO_FIXED_POINT
    print(f"[unstructured square, a = 0.4 / 0.5 / 1, rk4 coarsen {COARSEN}, ratios {[int(r) for r in c.ratios]}, f64 kernel 9, 12 WaveHoltz iterations] "
          f"{out.num_matvec} matvecs, distance to the exact-local-solve fixed point {e:.4e} (the restatement's flow "
          f"{RESTATEMENT_FLOW_TO_FIXED_POINT:.4e}, gate 2 x); the default plan (rk2, mesh grid): {e0:.4e}, {out0.num_matvec} matvecs, success {out0.success}")
    assert out.success, out.res_norm[-1] / out.res_norm[0]
    assert e <= gate, (e, gate)
