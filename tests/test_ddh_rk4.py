"""DDH(integrator="rk4", coarsen=c) without a GPU: the numpy restatement the GPU tests compare against (tests/ddh_rk.py) is pinned
to the oracle first, then used for what RK4 on a coarser grid is claimed to be (order, accuracy of the default, stability on the
mesh grid where RK2 blows up); then the host side of the product: the coarsened grid's tables, round trips, refusals.
Every distance is printed (`pytest -s`).

Figures of the order test (sweep case of tests/test_gpu_ddh_time_grids.py: 16 x 16 elements, n_basis 4, block 4, a == 1, fp64),
relative l2 distances of (rhs, action on the written slots, postprocess) between coarsen c and coarsen 1:
    d(2,1) = 1.54e-07 1.40e-07 1.82e-07     d(4,1) = 1.64e-06 1.81e-06 1.14e-06     d(8,1) = 2.97e-05 3.31e-05 1.43e-05
    d(4,1) / d(2,1) = 10.7 13.0 6.3 per output, 9.8 over the three (root of the sum of squares); d(8,1) / d(4,1) = 18.1 18.3 12.5
A fourth-order scheme gives 17 and a second-order one 5.  The figures lie between because the march is not RK4 alone: the filter
sums u += filt[it] p are the trapezoid rule of the period average, which the integrator does not touch, and its dt^2 term (small:
the integrand nearly closes over a period) shows once RK4's own error is as small as at coarsen 2.  postprocess, whose output is
the field on every dof and not the traces alone, carries most of it: alone it is at 6.3, below the 8 the joint figure is held to.
"""
import math

import numpy as np
import pytest

import ddh_rk as rk
import ddh_time_grids as tg
from test_baseline_regime import NB
from test_gpu_ddh_time_grids import RATIOS

NAMES = ("rhs", "action", "postprocess")
TIME_TABLES = ("filter", "cs", "sn")
ALL_TABLES = ("B", "gI", "sI", "D", "m", "gmi", "a", "H") + TIME_TABLES
STABLE_COARSEN = 2  # the coarsening of the stability claim; 1 would be the fallback if 2 were outside RK4's range at a = 0.2: it is not


def joint(ds):
    return math.sqrt(sum(x * x for x in ds))


# ===================================================================================================== the restatement
def test_restatement_in_rk2_mode_is_the_per_subdomain_oracle():
    """16 x 16 elements, n_basis 4, block 4, the GPU time-grid test's RATIOS: the restatement with the oracle's scheme against the
    oracle itself (once per subdomain on that subdomain's grid), fp64, 1e-12"""
    c = rk.sweep_case(4)
    P = tg.PerSubdomainOracle(c.O["f64"], RATIOS[4])
    ref = (P.rhs(c.fh), P.action(c.lam)[c.written], P.postprocess(c.lam, c.fh))
    got = rk.sweep_outputs(4, "rk2", 1, RATIOS[4])
    e = [rk.rel(a, b) for a, b in zip(got, ref)]
    for nm, x in zip(NAMES, e):
        print(f"[block 4, ratios {list(RATIOS[4])}, rk2 restatement] {nm}: vs per-subdomain fp64 oracle {x:.3e} (gate 1e-12)")
    assert all(np.linalg.norm(r) > 0 for r in ref)
    assert all(x <= 1e-12 for x in e), e


def test_rk4_restatement_is_of_higher_than_second_order():
    out = {c: rk.sweep_outputs(4, "rk4", c) for c in (1, 2, 4)}
    d2 = [rk.rel(a, b) for a, b in zip(out[2], out[1])]
    d4 = [rk.rel(a, b) for a, b in zip(out[4], out[1])]
    for nm, a, b in zip(NAMES, d4, d2):
        print(f"[block 4, a == 1, rk4 restatement] {nm}: d(4,1) {a:.3e}, d(2,1) {b:.3e}, ratio {a / b:.2f} (fourth order 17, second order 5)")
    ratio = joint(d4) / joint(d2)
    print(f"over the three outputs: {ratio:.2f} (gate: at least 8)")
    assert ratio >= 8, (ratio, d4, d2)


def test_rk4_at_coarsen_4_is_closer_to_the_exact_march_than_rk2_on_the_mesh_grid():
    """the reason for the default: distances to RK4 on twice the mesh grid's steps"""
    fine = rk.sweep_outputs(4, "rk4", 1, None, "f64", 2)
    e4 = [rk.rel(a, b) for a, b in zip(rk.sweep_outputs(4, "rk4", 4), fine)]
    e2 = [rk.rel(a, b) for a, b in zip(rk.sweep_outputs(4, "rk2", 1), fine)]
    for nm, a, b in zip(NAMES, e4, e2):
        print(f"[block 4, a == 1] {nm}: rk4 on nt_mesh / 4 (half the sweeps) {a:.3e}, rk2 on nt_mesh {b:.3e}, to rk4 on 2 nt_mesh")
    assert all(a < b for a, b in zip(e4, e2)), (e4, e2)


def test_rk4_restatement_is_stable_on_the_mesh_grid_where_rk2_is_not():
    """config 3's disk window (a = 0.2 in the disk, nt_mesh 5120), every subdomain on the one grid (ratios all 1), power iteration
    of tests/test_baseline_regime.py, seed 1, three steps: the RK2 oracle grows by 1e5 to 1e7 per step there
    (tests/test_ddh_time_grids.py), RK4 on the grid coarsened by 2 does not grow"""
    got = rk.stability_growth_rk4(STABLE_COARSEN)
    print(f"config 3 disk window, rk4 restatement, coarsen {STABLE_COARSEN}, ratios all 1: " + " ".join(f"{r:.6f}" for r in got))
    assert all(np.isfinite(r) and r <= 1.05 for r in got), got


# ===================================================================================================== host tables
def product(w, cd, precision="f32", **kw):
    mesh = cd.Mesh2D.uniform_rect(w.nw, w.x0, w.x1, w.nw, w.y0, w.y1)
    fem = cd.H1Space(mesh, cd.Basis(NB))
    return cd.DDH(w.omega, kw.pop("h_a", w.h_a), fem, w.nw, w.nw, precision=precision, **kw), fem


def host_info(F):
    return {k: v for k, v in F.info().items() if k != "kernel"}  # the kernel is the plan's, made on a GPU


@pytest.mark.parametrize("precision,real", [("f32", np.float32), ("f64", np.float64)])
def test_coarsened_grid_tables_are_the_restated_ones_bitwise(precision, real):
    import cuddhelmholtz_amd as cd

    w, O, _ = tg.stability_window()
    nt = math.ceil(O.t.nt / 3)
    assert O.t.nt % 3 != 0  # the ceiling is exercised
    F, _ = product(w, cd, precision, integrator="rk4", coarsen=3)
    assert F.integrator() == ("rk4", 3)
    assert F.info()["nt"] == nt and F.info()["dt"] == 2 * math.pi / w.omega / nt
    dt, filt, cs, sn = tg.time_grid(w.omega, nt, real)
    for name, ref in zip(TIME_TABLES, (filt, cs, sn)):
        got = F.table(name)
        assert got.dtype == ref.dtype and np.array_equal(got, ref), name
        assert np.array_equal(F.table(f"{name}@1"), ref), name
    assert list(F.time_ratios()) == [1, 1, 1, 1]
    # time_step composes: r times the coarsened count
    F, _ = product(w, cd, precision, integrator="rk4", coarsen=3, time_step=np.array([5, 1, 3, 1]))
    assert F.info()["nt"] == nt and list(F.time_ratios()) == [5, 1, 3, 1] and F.integrator() == ("rk4", 3)
    for r in (1, 3, 5):
        dt, filt, cs, sn = tg.time_grid(w.omega, r * nt, real)
        for name, ref in zip(TIME_TABLES, (filt, cs, sn)):
            got = F.table(f"{name}@{r}")
            assert got.dtype == ref.dtype and got.shape == ((r * nt + 1,) if name == "filter" else (2 * r * nt + 1,))
            assert np.array_equal(got, ref), (name, r)
    # the default coarsening, and coefficient ratios on top of it
    F, _ = product(w, cd, precision, integrator="rk4", time_step="coefficient")
    assert F.integrator() == ("rk4", 4) and F.info()["nt"] == O.t.nt // 4 and list(F.time_ratios()) == [5, 1, 5, 1]


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_rk2_is_the_plan_without_the_argument(precision):
    import cuddhelmholtz_amd as cd

    w, _, _ = tg.stability_window()
    F0, _ = product(w, cd, precision)
    assert F0.integrator() == ("rk2", 1)
    for kw in (dict(integrator="rk2"), dict(integrator="rk2", coarsen=1), dict(integrator="rk2", coarsen=None, time_step="mesh")):
        F, _ = product(w, cd, precision, **kw)
        assert F.integrator() == ("rk2", 1)
        assert host_info(F) == host_info(F0)
        for name in ALL_TABLES:
            assert np.array_equal(F.table(name), F0.table(name)), name
    # rk4 at coarsen 1 marches on the mesh grid's tables as well
    F, _ = product(w, cd, precision, integrator="rk4", coarsen=1)
    assert F.integrator() == ("rk4", 1) and host_info(F) == host_info(F0)
    for name in ALL_TABLES:
        assert np.array_equal(F.table(name), F0.table(name)), name


def test_integrator_refusals_come_before_anything_is_built():
    import cuddhelmholtz_amd as cd
    from cuddhelmholtz_amd import _native as N
    from cuddhelmholtz_amd.api import _h

    w, _, _ = tg.stability_window()
    for kw in (dict(integrator="rk3"), dict(integrator="RK4"), dict(integrator=4), dict(integrator=None),
               dict(integrator="rk4", coarsen=0), dict(integrator="rk4", coarsen=17), dict(integrator="rk4", coarsen=2.5),
               dict(integrator="rk4", coarsen=True), dict(integrator="rk4", coarsen=-4), dict(integrator="rk4", coarsen="4"),
               dict(integrator="rk2", coarsen=2), dict(coarsen=2), dict(integrator="rk2", coarsen=0), dict(integrator="rk2", coarsen=True)):
        with pytest.raises(ValueError):
            product(w, cd, **kw)
    for c in (1, 16, np.int32(8)):
        assert product(w, cd, integrator="rk4", coarsen=c)[0].integrator() == ("rk4", int(c))
    # the same checks in the C++ constructor, through the C creator, for callers that do not come through Python
    mesh = cd.Mesh2D.uniform_rect(w.nw, w.x0, w.x1, w.nw, w.y0, w.y1)
    fem = cd.H1Space(mesh, cd.Basis(NB))
    for integrator, coarsen in ((0, 2), (1, 0), (1, 17), (1, -1), (2, 1), (-1, 1), (0, 0)):
        assert not N.lib.cuddh_ddh_create_integrator(w.omega, _h(w.h_a), fem._h, w.nw, w.nw, 0, 0, 0, 0, None, 0, integrator, coarsen)
        assert N.last_error().startswith("DDH error: integrator"), N.last_error()
    h = N.lib.cuddh_ddh_create_integrator(w.omega, _h(w.h_a), fem._h, w.nw, w.nw, 0, 0, 0, 0, None, 0, 0, 1)  # rk2: the existing creator
    assert h
    N.lib.cuddh_ddh_destroy(h)
