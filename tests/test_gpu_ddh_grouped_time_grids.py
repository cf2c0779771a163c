"""DDH kernel 13 on the device: the element-lane local solves with four subdomains per wavefront on per-subdomain time
grids ("Kernel 13").  A wavefront marches once per distinct grid among its four rows; a row that is not on the
pass's grid takes the leader's subdomain and publishes nothing.

Shapes, a = 1, omega = 2 pi nx / 10, [-1,1]^2, blocks of 4 x 4 elements numbered as test_gpu_ddh_time_grids.block_labels:
  * n_basis 4: 16 x 16 elements, 16 subdomains, four wavefronts;
  * n_basis 5: 12 x 8 elements, 6 subdomains: one full wavefront and a tail of two rows.
Ratios R = [3,1,2,1, 1,1,1,1, 2,2,4,1, 1,3,1,2] (the first 6 at n_basis 5): in index order the wavefronts hold three grids,
one, three, three; in the plan's sorted order {4,3,3,2}, {2,2,2,1} and two of ones.

  1. parity of rhs / action / postprocess with both owner rules against the per-subdomain fp64 oracle, gate 4 x the distance
     of the fp32 per-subdomain oracle to it (the rule of test_fp32_parity_with_explicit_ratios);
  2. a subdomain's result does not depend on its wave-mates or its pass, bitwise: sorted full launch, ranges with tails of
     one and three rows, listed launches, a wavefront with four distinct grids, wave priority, a repeat;
  3. the right grid per row, bitwise: the plan with every subdomain on r against the mixed plan at the slots of R[s] == r;
  4. one grid is the existing code, bitwise: kernel 13 on the mesh grid against kernel 5's element-lane form / kernel 12, and
     the instantiations with time grids on ratios of one against those;
  5. stability on config 3's disk window under `coefficient`, the fp32 bounds of test_gpu_ddh_time_grids;
  6. refusals and selection.
Every distance is printed (`pytest -s`).
"""
import functools
import math

import numpy as np
import pytest

import ddh_general as dg
import ddh_time_grids as tg
import oracle
from test_baseline_regime import power_iteration
from test_gpu_ddh_time_grids import NAMES, block_labels, distances, entry_points
from test_gpu_parity import rel, to_dev

pytestmark = pytest.mark.gpu

R = (3, 1, 2, 1, 1, 1, 1, 1, 2, 2, 4, 1, 1, 3, 1, 2)
SHAPES = {4: (16, 16), 5: (12, 8)}  # n_basis: elements per side
BLOCK = 4


class Case:
    """inputs and per-subdomain oracle outputs of one shape; nothing in it is changed after construction"""

    def __init__(self, nb):
        self.nb = nb
        self.nx, self.ny = nx, ny = SHAPES[nb]
        self.omega = 2 * math.pi * nx / 10
        self.d = d = oracle.Discretization(oracle.Mesh.uniform_rect(nx, -1.0, 1.0, ny, -1.0, 1.0), nb)
        self.h_a = np.ones(d.ndof)
        self.fh = np.concatenate([oracle.linear_functional(d, oracle.gaussians(self.omega)), 0.1 * oracle.linear_functional(d, oracle.mass_poly)])
        self.n_domains = nd = (nx // BLOCK) * (ny // BLOCK)
        self.ratios = np.asarray(R[:nd], dtype=np.int32)
        labels = block_labels(nx, ny, BLOCK)
        O = dg.OracleDDH(d, nd, labels, self.omega, self.h_a, np.float64)
        self.size = n = O.size
        lam = np.random.default_rng(7).standard_normal(n)
        B = O.t.B
        used = np.unique(B[B >= 0])
        lam[np.setdiff1d(np.arange(n), np.concatenate([used, used + O.t.n_lambda]))] = 0.0
        self.lam = lam
        written = np.unique(B[:, 1, :][B[:, 1, :] >= 0])
        self.written = np.concatenate([written, written + O.t.n_lambda])
        self.ref = self.outputs_of(tg.PerSubdomainOracle(O, self.ratios))
        O32 = dg.OracleDDH(d, nd, labels, self.omega, self.h_a, np.float32)
        self.floor = tuple(rel(a, r) for a, r in zip(self.outputs_of(tg.PerSubdomainOracle(O32, self.ratios)), self.ref))

    def outputs_of(self, P):
        return P.rhs(self.fh), P.action(self.lam)[self.written], P.postprocess(self.lam, self.fh)


@functools.lru_cache(maxsize=None)
def case(nb):
    return Case(nb)


def make(cd, nb, kernel, time_step, form=None, **more):
    nx, ny = SHAPES[nb]
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, ny, -1.0, 1.0), cd.Basis(nb))
    F = cd.DDH(2 * math.pi * nx / 10, np.ones(fem.size()), fem, nx, ny, kernel=kernel, block=BLOCK, time_step=time_step, **more)
    if form is not None:
        F.set_sweep_form(form)
    assert F.info()["kernel"] == kernel
    return F


def forms(torch, cuda, F, ndof):
    """(name, x, lambda) of the three forms of a local solve: with x, with lambda, with both; the same values at every call"""
    rng = np.random.default_rng(11)
    x = to_dev(torch, rng.standard_normal(2 * ndof), cuda)
    lam = to_dev(torch, rng.standard_normal(F.size()).astype(np.float32), cuda)
    return (("x", x, None), ("lambda", None, lam), ("both", x, lam))


def traces(torch, cuda, F, x, lam, launches):
    """the trace vector after the given launches: (d0, d1) ranges or arrays of ids"""
    out = torch.zeros(F.size(), dtype=F.trace_dtype, device=cuda)
    for launch in launches:
        if isinstance(launch, tuple):
            F.local_traces(launch[0], launch[1], x, lam, out)
        else:
            F.local_traces_listed(to_dev(torch, np.asarray(launch, dtype=np.int32), cuda), x, lam, out)
    return out


def slots_of(F, subdomains):
    """the trace slots the given subdomains write (both halves of the vector), from the plan's own table"""
    info = F.info()
    B = F.table("B").reshape(info["n_domains"], 2, info["mx_fdof"])
    s = np.unique(B[np.asarray(subdomains, dtype=np.int64), 1, :])
    s = s[s >= 0]
    return np.concatenate([s, s + info["n_lambda"]])


@pytest.mark.parametrize("nb", [4, 5])
def test_parity_with_mixed_grids(cuda, nb):
    import torch

    import cuddhelmholtz_amd as cd

    c = case(nb)
    F = make(cd, nb, 13, c.ratios)
    assert F.info()["kernel"] == 13 and list(F.time_ratios()) == list(c.ratios) and F.size() == c.size
    for last in (False, True):
        F.set_owner_rule(last)
        e = distances(c, entry_points(torch, cuda, F, c.fh, c.lam, c.d.ndof))
        for nm, x, fl in zip(NAMES, e, c.floor):
            print(f"[n_basis {nb}, ratios {[int(r) for r in c.ratios]}, kernel 13, {'last' if last else 'first'} copy] {nm}: floor (fp32 per-subdomain "
                  f"oracle vs fp64) {fl:.3e}, gate 4 x; product vs fp64 oracle {x:.3e} ({x / fl:.2f} x floor)")
        for nm, x, fl in zip(NAMES, e, c.floor):
            assert x <= 4 * fl, (nm, last, x, 4 * fl)


@pytest.mark.parametrize("nb", [4, 5])
def test_result_does_not_depend_on_wave_mates_or_pass(cuda, nb):
    import torch

    import cuddhelmholtz_amd as cd

    c = case(nb)
    nd = c.n_domains
    F = make(cd, nb, 13, c.ratios)
    cuts = (0, 1, 9, nd) if nd == 16 else (0, 1, 5, 6)  # launches of 1, 8 and 7 (1, 4 and 1): tails of one and three rows
    perm = np.random.default_rng(3).permutation(nd).astype(np.int32)
    for name, x, lam in forms(torch, cuda, F, c.d.ndof):
        full = traces(torch, cuda, F, x, lam, [(0, nd)])  # the plan's order: longest first
        assert full.abs().max().item() > 0
        assert torch.equal(traces(torch, cuda, F, x, lam, list(zip(cuts[:-1], cuts[1:]))), full), name
        assert torch.equal(traces(torch, cuda, F, x, lam, [perm[: nd // 3], perm[nd // 3:]]), full), name
        if nb == 4:  # a wavefront whose rows are on grids 4, 3, 2, 1: four passes
            first = [10, 0, 2, 1]
            assert sorted(c.ratios[first]) == [1, 2, 3, 4]
            assert torch.equal(traces(torch, cuda, F, x, lam, [first + [s for s in range(nd) if s not in first]]), full), name
        F.set_wave_priority(True)
        assert torch.equal(traces(torch, cuda, F, x, lam, [(0, nd)]), full), name
        F.set_wave_priority(False)
        assert torch.equal(traces(torch, cuda, F, x, lam, [(0, nd)]), full), name


@pytest.mark.parametrize("nb", [4, 5])
def test_every_row_marches_on_its_own_grid(cuda, nb):
    import torch

    import cuddhelmholtz_amd as cd

    c = case(nb)
    nd = c.n_domains
    F = make(cd, nb, 13, c.ratios)
    mixed = {name: traces(torch, cuda, F, x, lam, [(0, nd)]) for name, x, lam in forms(torch, cuda, F, c.d.ndof)}
    seen = 0
    for r in sorted(set(int(v) for v in c.ratios)):
        Fr = make(cd, nb, 13, np.full(nd, r, dtype=np.int32))
        mine = torch.from_numpy(slots_of(Fr, np.flatnonzero(c.ratios == r))).to(cuda)
        assert mine.numel() > 0
        seen += mine.numel()
        for name, x, lam in forms(torch, cuda, Fr, c.d.ndof):
            one = traces(torch, cuda, Fr, x, lam, [(0, nd)])
            assert one[mine].abs().max().item() > 0
            assert torch.equal(one[mine], mixed[name][mine]), (name, r)
    assert seen == slots_of(F, np.arange(nd)).size  # every written slot was compared, each under one ratio


@pytest.mark.parametrize("nb", [4, 5])
def test_one_grid_is_the_existing_code(cuda, nb):
    import torch

    import cuddhelmholtz_amd as cd

    c = case(nb)
    old = make(cd, 4, 5, "mesh", form=2) if nb == 4 else make(cd, 5, 12, "mesh")
    mesh = make(cd, nb, 13, "mesh")
    ones = make(cd, nb, 13, np.ones(c.n_domains, dtype=np.int32))
    assert list(ones.time_ratios()) == [1] * c.n_domains
    want = entry_points(torch, cuda, old, c.fh, c.lam, c.d.ndof)
    for F in (mesh, ones):  # the one-grid kernels themselves; the instantiations with time grids on one grid
        for nm, a, b in zip(NAMES, want, entry_points(torch, cuda, F, c.fh, c.lam, c.d.ndof)):
            assert a.abs().max().item() > 0
            assert torch.equal(a, b), nm


def test_product_is_stable_on_the_disk_window(cuda):
    """config 3's disk window (tests/test_baseline_regime.py: |T| ~ 1e7 on the mesh grid) under `coefficient` on kernel 13"""
    import torch

    import cuddhelmholtz_amd as cd

    w, O, ratios = tg.stability_window()
    ref = tg.stability_growth_per_subdomain()
    assert 0.9 < ref[-1] < 1.05
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(w.nw, w.x0, w.x1, w.nw, w.y0, w.y1), cd.Basis(4))
    F = cd.DDH(w.omega, w.h_a, fem, w.nw, w.nw, kernel=13, block=4, time_step="coefficient")
    assert F.info()["kernel"] == 13 and list(F.time_ratios()) == list(ratios) == [5, 1, 5, 1]
    nd = F.info()["n_domains"]

    def T(v):
        lam = torch.from_numpy(np.ascontiguousarray(v)).to(cuda).to(F.trace_dtype)
        out = torch.zeros_like(lam)
        F.local_traces(0, nd, None, lam, out)
        return out.double().cpu().numpy()

    got = power_iteration(T, F.size(), tg.STABILITY_STEPS, seed=1)
    print(f"config 3 disk window, coefficient ratios {[int(r) for r in ratios]}, f32 kernel 13: " + " ".join(f"{r:.6f}" for r in got)
          + " (per-subdomain oracle " + " ".join(f"{r:.6f}" for r in ref) + ")")
    assert 0.9 < got[-1] < 1.05
    assert abs(got[-1] - ref[-1]) <= 2e-3 * ref[-1]


def test_refusals_and_selection(cuda):
    import cuddhelmholtz_amd as cd

    def ddh(nb, nx, block, kernel, time_step="mesh", **more):
        fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), cd.Basis(nb))
        return cd.DDH(2 * math.pi * nx / 10, np.ones(fem.size()), fem, nx, nx, kernel=kernel, block=block, time_step=time_step, **more)

    for nb, nx, block, more in ((4, 16, 8, {}), (5, 8, 2, {}), (4, 16, 4, {"precision": "f64"}), (4, 16, 4, {"integrator": "rk4"}),
                                (5, 8, 4, {"integrator": "rk4"}), (8, 4, None, {})):
        with pytest.raises(RuntimeError):
            ddh(nb, nx, block, 13, **more).info()
    r16 = np.asarray(R, dtype=np.int32)
    for F in (ddh(4, 16, 4, 13), ddh(4, 16, 4, 13, r16), ddh(5, 8, 4, 13), ddh(5, 8, 4, 13, r16[:4])):
        assert F.info()["kernel"] == 13 and F.sweep_form() == 0
        with pytest.raises(RuntimeError):
            F.set_sweep_form(2)
        assert F.sweep_form() == 0
        F.set_owner_rule(True)
        F.set_owner_rule(False)
    # what a plan with grids ran before kernel 13 existed, it runs now
    F = ddh(4, 16, 4, 0, r16)
    assert F.info()["kernel"] == 5 and F.sweep_form() == 1
    r64 = np.ones(64, dtype=np.int32)
    r64[::3] = 2
    assert ddh(5, 32, 4, 0, r64).info()["kernel"] == 1 and ddh(5, 32, 4, 0).info()["kernel"] == 12
    with pytest.raises(RuntimeError):
        ddh(5, 8, 4, 12, r16[:4]).info()
    with pytest.raises(RuntimeError):
        ddh(4, 16, 4, 5, r16).set_sweep_form(2)
