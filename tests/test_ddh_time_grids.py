"""DDH(time_step=...) on the host: ratios, per-grid tables, what collapses to the default plan, refusals; and, on the oracle alone,
why it exists (the power iteration of DESIGN 5.2 on config 3's disk window: |T| ~ 1e7 on the mesh grid, ~1 per subdomain).
Nothing here needs a GPU: the time grids are host tables like every other DDH table.
"""
import math

import numpy as np
import pytest

import ddh_time_grids as tg
import oracle
from test_baseline_regime import NB, power_iteration

TIME_TABLES = ("filter", "cs", "sn")
ALL_TABLES = ("B", "gI", "sI", "D", "m", "gmi", "a", "H") + TIME_TABLES


def product(w, cd, precision="f32", **kw):
    mesh = cd.Mesh2D.uniform_rect(w.nw, w.x0, w.x1, w.nw, w.y0, w.y1)
    fem = cd.H1Space(mesh, cd.Basis(NB))
    return cd.DDH(w.omega, kw.pop("h_a", w.h_a), fem, w.nw, w.nw, precision=precision, **kw), fem


def host_info(F):
    return {k: v for k, v in F.info().items() if k != "kernel"}  # the kernel is the plan's, made on a GPU


def test_coefficient_ratios_on_the_disk_window():
    import cuddhelmholtz_amd as cd

    w, O, want = tg.stability_window()
    assert list(want) == [5, 1, 5, 1]
    F, _ = product(w, cd, time_step="coefficient")
    assert list(F.time_ratios()) == [5, 1, 5, 1]
    assert F.info()["nt"] == O.t.nt == 5120 and F.info()["dt"] == O.t.dt  # the base grid stays the mesh grid
    F0, _ = product(w, cd)
    assert list(F0.time_ratios()) == [1, 1, 1, 1]


@pytest.mark.parametrize("precision,real", [("f32", np.float32), ("f64", np.float64)])
def test_per_grid_tables_are_the_restated_ones_bitwise(precision, real):
    import cuddhelmholtz_amd as cd

    w, O, _ = tg.stability_window()
    F, _ = product(w, cd, precision, time_step=np.array([5, 1, 3, 1]))
    assert list(F.time_ratios()) == [5, 1, 3, 1]
    for r in (1, 3, 5):
        dt, filt, cs, sn = tg.time_grid(w.omega, r * O.t.nt, real)
        for name, ref in zip(TIME_TABLES, (filt, cs, sn)):
            got = F.table(f"{name}@{r}")
            assert got.dtype == ref.dtype and got.shape == ref.shape == ((r * O.t.nt + 1,) if name == "filter" else (2 * r * O.t.nt + 1,))
            assert np.array_equal(got, ref), (name, r)
    # the base grid's tables stay what they were, and a grid nobody marches on is not there
    F0, _ = product(w, cd, precision)
    for name in TIME_TABLES:
        assert np.array_equal(F.table(name), F0.table(name))
    with pytest.raises(RuntimeError):
        F.table("filter@2")
    with pytest.raises(RuntimeError):
        F.table("gI@1")


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_mesh_and_coefficient_with_a_one_are_the_default_plan(precision):
    import cuddhelmholtz_amd as cd

    w, _, _ = tg.stability_window()
    ones = np.ones(w.ndof)
    F0, _ = product(w, cd, precision, h_a=ones)
    for kw in (dict(time_step="mesh"), dict(time_step="coefficient"), dict(time_step="coefficient", block=4)):
        F, _ = product(w, cd, precision, h_a=ones, **kw)
        assert host_info(F) == host_info(F0)
        assert list(F.time_ratios()) == [1, 1, 1, 1]
        for name in ALL_TABLES:
            assert np.array_equal(F.table(name), F0.table(name)), name
        for name in TIME_TABLES:
            assert np.array_equal(F.table(f"{name}@1"), F0.table(name))
    # a >= 1 is never coarsened
    F, _ = product(w, cd, precision, h_a=np.full(w.ndof, 3.0), time_step="coefficient")
    assert list(F.time_ratios()) == [1, 1, 1, 1] and F.info()["nt"] == F0.info()["nt"]


@pytest.mark.parametrize("precision,real", [("f32", np.float32), ("f64", np.float64)])
def test_coefficient_with_one_ratio_is_one_grid(precision, real):
    import cuddhelmholtz_amd as cd

    w, O, _ = tg.stability_window()
    F, _ = product(w, cd, precision, h_a=np.full(w.ndof, 0.5), time_step="coefficient")
    nt0 = O.t.nt
    assert list(F.time_ratios()) == [2, 2, 2, 2]
    assert F.info()["nt"] == 2 * nt0 and F.info()["dt"] == 2 * math.pi / w.omega / (2 * nt0)
    dt, filt, cs, sn = tg.time_grid(w.omega, 2 * nt0, real)
    for name, ref in zip(TIME_TABLES, (filt, cs, sn)):
        assert np.array_equal(F.table(name), ref) and np.array_equal(F.table(f"{name}@2"), ref)
    with pytest.raises(RuntimeError):
        F.table("filter@1")
    # 1 / a an integer up to rounding stays on that integer, just above it takes the next
    for a, r in ((0.2, 5), (1 / 3, 3), (0.19, 6), (0.9999, 2)):
        F, _ = product(w, cd, precision, h_a=np.full(w.ndof, a), time_step="coefficient")
        assert list(F.time_ratios()) == [r] * 4, (a, r)


def test_refusals_come_before_anything_is_built():
    import cuddhelmholtz_amd as cd

    w, _, _ = tg.stability_window()
    bad_a = []
    for v in (float("nan"), float("inf"), 0.0, -0.2):
        a = w.h_a.copy()
        a[w.ndof // 2] = v
        bad_a.append(a)
    bad_a.append(np.full(w.ndof, 1 / 257))  # ratio 257
    for a in bad_a:
        with pytest.raises(ValueError):
            product(w, cd, h_a=a, time_step="coefficient")
    assert list(product(w, cd, h_a=np.full(w.ndof, 1 / 256), time_step="coefficient")[0].time_ratios()) == [256] * 4
    for ratios in ([1, 2, 3], [1, 2, 3, 4, 5], [], [1, 0, 1, 1], [1, -2, 1, 1], [1, 257, 1, 1], [1.0, 2.0, 1.0, 1.0], [[1, 2], [1, 1]]):
        with pytest.raises(ValueError):
            product(w, cd, time_step=np.array(ratios))
    with pytest.raises(ValueError):
        product(w, cd, time_step="finest")
    # the same array checks in the C++ constructor, for callers that do not come through Python
    from cuddhelmholtz_amd import _native as N
    from cuddhelmholtz_amd.api import _h

    mesh = cd.Mesh2D.uniform_rect(w.nw, w.x0, w.x1, w.nw, w.y0, w.y1)
    fem = cd.H1Space(mesh, cd.Basis(NB))
    for ratios in ([1, 2, 3], [1, 0, 1, 1], [1, 257, 1, 1]):
        r = np.array(ratios, dtype=np.int32)
        assert not N.lib.cuddh_ddh_create_timegrid(w.omega, _h(w.h_a), fem._h, w.nw, w.nw, 0, 0, 0, 2, _h(r), r.size)
        assert N.last_error().startswith("DDH error: time step")
    assert not N.lib.cuddh_ddh_create_timegrid(w.omega, _h(w.h_a), fem._h, w.nw, w.nw, 0, 0, 0, 3, None, 0)
    # subdomains from labels march on the mesh grid
    labels = np.arange(w.nw * w.nw, dtype=np.int32) // 16
    with pytest.raises(ValueError):
        cd.DDH.from_labels(w.omega, w.h_a, fem, labels, time_step="coefficient")
    with pytest.raises(ValueError):
        cd.DDH.from_labels(w.omega, w.h_a, fem, labels, time_step=np.ones(4, dtype=np.int32))
    assert cd.DDH.from_labels(w.omega, w.h_a, fem, labels, time_step="mesh").info()["n_domains"] == 4


def test_oracle_local_solves_are_stable_on_per_subdomain_grids():
    """The power iteration of tests/test_baseline_regime.py on config 3's disk window (8 x 8 elements, seed 1, three steps), fp64
    oracle: on the mesh grid the last growth factor is ~1e7, with every subdomain on the grid of its own coefficient it is the
    a == 1 behaviour."""
    w, O, ratios = tg.stability_window()
    mesh_grid = power_iteration(lambda v: O.solve(lam=v)[1], O.size, tg.STABILITY_STEPS, seed=1)
    own = tg.stability_growth_per_subdomain()
    print("mesh grid: " + " ".join(f"{r:.3e}" for r in mesh_grid) + " | per subdomain " + str([int(r) for r in ratios]) + ": " + " ".join(f"{r:.4f}" for r in own))
    assert mesh_grid[-1] > 1e5
    assert 0.9 < own[-1] < 1.05
    assert (O.t.nt, len(O.t.wh_filter)) == (5120, 5121)  # the oracle's tables are back in place
