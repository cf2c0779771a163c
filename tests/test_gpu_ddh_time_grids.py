"""DDH(time_step=...) on the device: every subdomain marches its WaveHoltz period on its own time grid.

Shapes: 16 x 16 elements on [-1,1]^2, n_basis 4, omega = 2 pi nx / 10 (mesh grid: nt about 800).  Blocks of 4 x 4 give 16
subdomains, with ratios that put four different step counts into the wavefronts of one workgroup of the wavefront kernels,
in a sorted full launch and in a range launch alike; blocks of 8 x 8 give 4 subdomains with four different ratios in kernel
11's one workgroup.  The reference is tests/ddh_time_grids.PerSubdomainOracle (the oracle's own local solve, once per
subdomain on that subdomain's grid), computed once per case and shared.

  * parity of rhs / action (written slots) / postprocess: fp64 kernels 1, 2, 3, 8 (and 1 at block 8) at 1e-10, the project's
    fp64 gate; fp32 kernels 1, 3, 5 (matrix form) and 11 at 4 x the distance of the fp32 per-subdomain oracle to the fp64 one,
    computed here (the floor rule of tests/test_gpu_ddh_block_size.py); the example's disk coefficient with the ratios of the
    `coefficient` policy, fp64 at 1e-10 (the steps are within the stable range there, DESIGN 5.2, so the gate is the plain one);
  * bitwise: explicit ratios of 1 (the instantiations with time grids) against the default plan; explicit ratios of 2 against
    `coefficient` on a = 0.5 (the plain kernels on the grid of 2 nt steps); the full launch (longest solves first) against
    ranges plus scrambled lists;
  * stability: config 3's disk window of tests/test_baseline_regime.py under `coefficient`: the growth factor of the power
    iteration is the per-subdomain oracle's, ~1 where the mesh grid gives ~1e7;
  * selection and refusals of the kernels that hold several subdomains per wavefront;
  * physics: a varying coefficient, 20 WaveHoltz iterations, rhs -> GMRES -> postprocess against ddh_general.fixed_point.
Every distance is printed (`pytest -s`).
"""
import functools
import math

import numpy as np
import pytest

import ddh_general as dg
import ddh_time_grids as tg
import oracle
from test_baseline_regime import NB, power_iteration
from test_gpu_parity import rel, to_dev

pytestmark = pytest.mark.gpu

NAMES = ("rhs", "action", "postprocess")
FP64_GATE = 1e-10
NX = 16
RATIOS = {4: (1, 2, 3, 1, 5, 1, 1, 2, 1, 1, 2, 1, 1, 3, 1, 1), 8: (1, 2, 3, 4)}
# distance of the per-subdomain oracle's own flow (20 WaveHoltz iterations, GMRES(120) to 1e-6) to ddh_general.fixed_point on
# tests/ddh_time_grids.physics_case, measured once on the CPU with
#   python profiles/tools/ddh_time_grid_oracle_flow.py 20        (114 matvecs; the same flow on the mesh grid: 3.2262e-05)
ORACLE_FLOW_TO_FIXED_POINT = 5.8895e-06


def block_labels(nx, ny, block):
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    return ((i // block) + (nx // block) * (j // block)).reshape(-1).astype(np.int32)


class Case:
    """inputs and per-subdomain oracle outputs of one decomposition; nothing in it is changed after construction"""

    def __init__(self, block, coef, with_f32):
        self.block = block
        self.omega = 2 * math.pi * NX / 10
        self.d = d = oracle.Discretization(oracle.Mesh.uniform_rect(NX, -1.0, 1.0, NX, -1.0, 1.0), NB)
        self.h_a = d.nodal(oracle.alpha_disk) if coef == "disk" else np.ones(d.ndof)
        self.fh = np.concatenate([oracle.linear_functional(d, oracle.gaussians(self.omega)), 0.1 * oracle.linear_functional(d, oracle.mass_poly)])
        self.n_domains = (NX // block) ** 2
        labels = block_labels(NX, NX, block)
        O = dg.OracleDDH(d, self.n_domains, labels, self.omega, self.h_a, np.float64)
        self.nt0, self.size = O.t.nt, O.size
        self.ratios = np.asarray(RATIOS[block] if coef == "one" else tg.coefficient_ratios(O.t, self.h_a), dtype=np.int32)
        n = O.size
        lam = np.random.default_rng(7).standard_normal(n)
        B = O.t.B
        used = np.unique(B[B >= 0])
        lam[np.setdiff1d(np.arange(n), np.concatenate([used, used + O.t.n_lambda]))] = 0.0
        self.lam = lam
        written = np.unique(B[:, 1, :][B[:, 1, :] >= 0])
        self.written = np.concatenate([written, written + O.t.n_lambda])
        self.ref = self.outputs_of(tg.PerSubdomainOracle(O, self.ratios))
        self.floor = None
        if with_f32:
            O32 = dg.OracleDDH(d, self.n_domains, labels, self.omega, self.h_a, np.float32)
            self.floor = tuple(rel(a, r) for a, r in zip(self.outputs_of(tg.PerSubdomainOracle(O32, self.ratios)), self.ref))

    def outputs_of(self, P):
        return P.rhs(self.fh), P.action(self.lam)[self.written], P.postprocess(self.lam, self.fh)


@functools.lru_cache(maxsize=None)
def case(block, coef="one", with_f32=True):
    return Case(block, coef, with_f32)


def make(cd, block, precision, kernel, time_step, h_a=None, form=None):
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(NX, -1.0, 1.0, NX, -1.0, 1.0), cd.Basis(NB))
    h_a = np.ones(fem.size()) if h_a is None else h_a
    F = cd.DDH(2 * math.pi * NX / 10, h_a, fem, NX, NX, precision=precision, kernel=kernel, block=block, time_step=time_step)
    if form is not None:
        F.set_sweep_form(form)
    assert F.info()["kernel"] == kernel
    return F, fem


def entry_points(torch, cuda, F, fh, lam_h, ndof):
    """(rhs, action, postprocess) as device tensors"""
    f = to_dev(torch, fh, cuda)
    lam = to_dev(torch, lam_h.astype(np.float64 if F.f64 else np.float32), cuda)
    b = torch.zeros(F.size(), dtype=F.trace_dtype, device=cuda)
    F.rhs(f, b)
    y = torch.zeros_like(b)
    F.action(lam, y)
    u = torch.zeros(2 * ndof, dtype=torch.float64, device=cuda)
    F.postprocess(lam, f, u)
    return b, y, u


def distances(c, out):
    b, y, u = (t.cpu().numpy().astype(np.float64) for t in out)
    return tuple(rel(a, r) for a, r in zip((b, y[c.written], u), c.ref))


# (precision, kernel, block, sweep form)
FP64 = [("f64", 1, 4, None), ("f64", 2, 4, None), ("f64", 3, 4, None), ("f64", 8, 4, None), ("f64", 1, 8, None)]
FP32 = [("f32", 1, 4, None), ("f32", 3, 4, None), ("f32", 5, 4, 1), ("f32", 11, 8, None), ("f32", 1, 8, None)]


@pytest.mark.parametrize("precision,kernel,block,form", FP64)
def test_fp64_parity_with_explicit_ratios(cuda, precision, kernel, block, form):
    import torch

    import cuddhelmholtz_amd as cd

    c = case(block)
    F, _ = make(cd, block, precision, kernel, c.ratios, form=form)
    assert list(F.time_ratios()) == list(c.ratios) and F.info()["nt"] == c.nt0 and F.size() == c.size
    e = distances(c, entry_points(torch, cuda, F, c.fh, c.lam, c.d.ndof))
    for nm, x in zip(NAMES, e):
        print(f"[block {block}, ratios {list(c.ratios)}, f64 kernel {kernel}] {nm}: vs per-subdomain fp64 oracle {x:.3e} (gate {FP64_GATE:.0e})")
    assert all(x <= FP64_GATE for x in e), e


@pytest.mark.parametrize("precision,kernel,block,form", FP32)
def test_fp32_parity_with_explicit_ratios(cuda, precision, kernel, block, form):
    import torch

    import cuddhelmholtz_amd as cd

    c = case(block)
    F, _ = make(cd, block, precision, kernel, c.ratios, form=form)
    assert list(F.time_ratios()) == list(c.ratios)
    if kernel == 5:
        assert F.sweep_form() == 1
    e = distances(c, entry_points(torch, cuda, F, c.fh, c.lam, c.d.ndof))
    for nm, x, fl in zip(NAMES, e, c.floor):
        print(f"[block {block}, ratios {list(c.ratios)}, f32 kernel {kernel}] {nm}: floor (fp32 per-subdomain oracle vs fp64) {fl:.3e}, gate 4 x; "
              f"product vs fp64 oracle {x:.3e} ({x / fl:.2f} x floor)")
    for nm, x, fl in zip(NAMES, e, c.floor):
        assert x <= 4 * fl, (nm, x, 4 * fl)


def test_disk_coefficient_with_coefficient_ratios(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    c = case(4, "disk", False)
    assert sorted(set(c.ratios)) == [1, 5] and 0 < int((c.ratios == 5).sum()) < 16  # the disk touches some subdomains, not all
    for kernel in (2, 8):
        F, _ = make(cd, 4, "f64", kernel, "coefficient", h_a=c.h_a)
        assert list(F.time_ratios()) == list(c.ratios) and F.info()["nt"] == c.nt0
        e = distances(c, entry_points(torch, cuda, F, c.fh, c.lam, c.d.ndof))
        for nm, x in zip(NAMES, e):
            print(f"[block 4, disk coefficient, ratios {list(c.ratios)}, f64 kernel {kernel}] {nm}: vs per-subdomain fp64 oracle {x:.3e} (gate {FP64_GATE:.0e})")
        assert all(x <= FP64_GATE for x in e), e


@pytest.mark.parametrize("precision,kernel,block,form", [("f32", 1, 4, None), ("f32", 3, 4, None), ("f32", 5, 4, 1), ("f64", 8, 4, None),
                                                         ("f32", 11, 8, None), ("f64", 1, 8, None)])
def test_ratios_of_one_are_bitwise_the_default_plan(cuda, precision, kernel, block, form):
    """the instantiations with time grids on one grid against the plain ones: the same arithmetic in the same order"""
    import torch

    import cuddhelmholtz_amd as cd

    c = case(block)
    F0, _ = make(cd, block, precision, kernel, "mesh", form=form)
    F1, _ = make(cd, block, precision, kernel, np.ones(c.n_domains, dtype=np.int32), form=form)
    if kernel == 5:  # what only a plan with time grids refuses: the explicit array was honoured, not collapsed
        with pytest.raises(RuntimeError):
            F1.set_sweep_form(2)
        assert F1.sweep_form() == 1
    for nm, a, b in zip(NAMES, entry_points(torch, cuda, F0, c.fh, c.lam, c.d.ndof), entry_points(torch, cuda, F1, c.fh, c.lam, c.d.ndof)):
        assert a.abs().max().item() > 0
        assert torch.equal(a, b), nm


@pytest.mark.parametrize("precision,kernel,block", [("f32", 5, 4), ("f64", 2, 4), ("f32", 11, 8)])
def test_ratios_of_two_are_bitwise_coefficient_one_half(cuda, precision, kernel, block):
    """per-subdomain instantiations on the grid of 2 nt steps against `coefficient` on a = 0.5, which is a plain plan on that grid"""
    import torch

    import cuddhelmholtz_amd as cd

    c = case(block)
    half = np.full(c.d.ndof, 0.5)
    Fc, _ = make(cd, block, precision, kernel, "coefficient", h_a=half)
    Fe, _ = make(cd, block, precision, kernel, np.full(c.n_domains, 2, dtype=np.int32), h_a=half)
    assert Fc.info()["nt"] == 2 * c.nt0 and Fe.info()["nt"] == c.nt0
    assert list(Fc.time_ratios()) == list(Fe.time_ratios()) == [2] * c.n_domains
    for nm, a, b in zip(NAMES, entry_points(torch, cuda, Fc, c.fh, c.lam, c.d.ndof), entry_points(torch, cuda, Fe, c.fh, c.lam, c.d.ndof)):
        assert a.abs().max().item() > 0
        assert torch.equal(a, b), nm


@pytest.mark.parametrize("precision,kernel,block,form", [("f32", 5, 4, 1), ("f32", 3, 4, None), ("f64", 1, 4, None), ("f32", 11, 8, None)])
def test_launch_partitions_are_bitwise_the_sorted_full_launch(cuda, precision, kernel, block, form):
    import torch

    import cuddhelmholtz_amd as cd

    c = case(block)
    F, _ = make(cd, block, precision, kernel, c.ratios, form=form)
    nd = c.n_domains
    f = to_dev(torch, c.fh, cuda)
    lam = to_dev(torch, c.lam.astype(np.float64 if F.f64 else np.float32), cuda)
    perm = np.random.default_rng(3).permutation(nd).astype(np.int32)
    cuts = (0, 1, nd // 2 + 1, nd)
    for x, l in ((f, None), (None, lam), (f, lam)):
        full = torch.zeros(F.size(), dtype=F.trace_dtype, device=cuda)
        F.local_traces(0, nd, x, l, full)  # the plan's order: longest first
        assert full.abs().max().item() > 0
        ranged = torch.zeros_like(full)
        for d0, d1 in zip(cuts[:-1], cuts[1:]):
            F.local_traces(d0, d1, x, l, ranged)
        assert torch.equal(ranged, full)
        listed = torch.zeros_like(full)
        for ids in (perm[: nd // 3], perm[nd // 3:]):
            F.local_traces_listed(to_dev(torch, ids, cuda), x, l, listed)
        assert torch.equal(listed, full)


def test_product_is_stable_on_the_disk_window_with_coefficient_ratios(cuda):
    """config 3's disk window (tests/test_baseline_regime.py: |T| ~ 1e7 on the mesh grid) under `coefficient`"""
    import torch

    import cuddhelmholtz_amd as cd

    w, O, ratios = tg.stability_window()
    ref = tg.stability_growth_per_subdomain()
    assert 0.9 < ref[-1] < 1.05
    for precision, kernel in (("f64", 2), ("f32", 5)):
        mesh = cd.Mesh2D.uniform_rect(w.nw, w.x0, w.x1, w.nw, w.y0, w.y1)
        fem = cd.H1Space(mesh, cd.Basis(NB))
        F = cd.DDH(w.omega, w.h_a, fem, w.nw, w.nw, precision=precision, kernel=kernel, time_step="coefficient")
        assert F.info()["kernel"] == kernel and list(F.time_ratios()) == list(ratios) == [5, 1, 5, 1] and F.info()["nt"] == 5120
        nd, tt = F.info()["n_domains"], F.trace_dtype

        def T(v):
            lam = torch.from_numpy(np.ascontiguousarray(v)).to(cuda).to(tt)
            out = torch.zeros_like(lam)
            F.local_traces(0, nd, None, lam, out)
            return out.double().cpu().numpy()

        got = power_iteration(T, F.size(), tg.STABILITY_STEPS, seed=1)
        print(f"config 3 disk window, coefficient ratios {[int(r) for r in ratios]}, {precision} kernel {kernel}: " + " ".join(f"{r:.6f}" for r in got)
              + " (per-subdomain oracle " + " ".join(f"{r:.6f}" for r in ref) + ")")
        assert 0.9 < got[-1] < 1.05
        assert abs(got[-1] - ref[-1]) <= (1e-9 if precision == "f64" else 2e-3) * ref[-1]


def test_selection_and_refusals_with_time_grids(cuda):
    import cuddhelmholtz_amd as cd

    # 8,192 subdomains: the size at which auto takes kernel 5's element-lane form (four subdomains per wavefront) on one grid
    nx, ny = 512, 256
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, ny, -1.0, 1.0), cd.Basis(4))
    ratios = np.ones(8192, dtype=np.int32)
    ratios[::7] = 2
    F = cd.DDH(16 * math.pi, np.ones(fem.size()), fem, nx, ny, time_step=ratios)
    assert F.info()["kernel"] == 5 and F.info()["n_domains"] == 8192
    assert F.sweep_form() == 1
    for form in (2, 3):
        with pytest.raises(RuntimeError):
            F.set_sweep_form(form)
    F.set_sweep_form(1)
    F.set_sweep_form(0)
    assert F.sweep_form() == 1
    del F

    # n_basis 8, blocks of 2 x 2 elements: kernels 6 and 7 hold two subdomains per wavefront
    fem8 = cd.H1Space(cd.Mesh2D.uniform_rect(4, -1.0, 1.0, 4, -1.0, 1.0), cd.Basis(8))
    ones8 = np.ones(fem8.size())

    def ddh8(precision, kernel, time_step):
        return cd.DDH(2 * math.pi * 4 / 10, ones8, fem8, 4, 4, precision=precision, kernel=kernel, time_step=time_step)

    r8 = np.array([1, 2, 1, 1], dtype=np.int32)
    assert ddh8("f32", 0, "mesh").info()["kernel"] == 7 and ddh8("f64", 0, "mesh").info()["kernel"] == 6  # today's choices
    assert ddh8("f32", 0, r8).info()["kernel"] == 1 and ddh8("f64", 0, r8).info()["kernel"] == 1
    for precision, kernel in (("f32", 7), ("f32", 6), ("f64", 6)):
        with pytest.raises(RuntimeError):
            ddh8(precision, kernel, r8).info()
        assert ddh8(precision, kernel, "mesh").info()["kernel"] == kernel


def test_physics_varying_coefficient_converges_to_the_exact_local_solve_fixed_point(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    d, omega, h_a, fh, labels, n_domains, O, ratios = tg.physics_case()
    assert list(ratios) == [3, 2, 3, 2]
    want = dg.fixed_point(O.t, O.G, d.ndof, fh)
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(8, -1.0, 1.0, 8, -1.0, 1.0), cd.Basis(NB))
    F = cd.DDH(omega, h_a, fem, 8, 8, precision="f64", time_step="coefficient")
    assert list(F.time_ratios()) == [3, 2, 3, 2] and F.info()["kernel"] == 3
    F.set_wh_iters(20)
    n = F.size()
    f = to_dev(torch, fh, cuda)
    b = torch.zeros(n, dtype=F.trace_dtype, device=cuda)
    lam = torch.zeros_like(b)
    u = torch.zeros(2 * d.ndof, dtype=torch.float64, device=cuda)
    F.rhs(f, b)
    out = cd.gmres(n, lam, F, b, 120, 30, 1e-6)
    assert out.success, out.res_norm[-1] / out.res_norm[0]
    F.postprocess(lam, f, u)
    e = rel(u.cpu().numpy(), want)
    gate = 2 * ORACLE_FLOW_TO_FIXED_POINT
    print(f"[8x8, a from 0.4 to 1, ratios {[int(r) for r in ratios]}, f64, 20 WaveHoltz iterations] {out.num_matvec} matvecs, distance to the "
          f"exact-local-solve fixed point {e:.4e} (the per-subdomain oracle's flow {ORACLE_FLOW_TO_FIXED_POINT:.4e}, gate 2 x)")
    assert e <= gate, (e, gate)
