"""DDH.from_labels(integrator=, coarsen=, time_ratios=) without a GPU: the host side (ratios, the coarsened base grid, the
per-grid tables, what collapses to the default plan, refusals in Python and in the C constructor), and the numpy restatement
pinned to the per-subdomain oracle on irregular labels before tests/test_gpu_ddh_labels_rk4.py relies on it.  The case is
tests/ddh_labels_rk.py: the reference's unstructured square, Morton parts of at most 16 elements plus the star of a valence-5
vertex, `coefficient` ratios 1, 2, 3.
Every distance is printed (`pytest -s`)."""
import numpy as np
import pytest

import ddh_labels_rk as lr
import ddh_rk as rk
import ddh_time_grids as tg

NAMES = ("rhs", "action", "postprocess")
TIME_TABLES = ("filter", "cs", "sn")
ALL_TABLES = ("B", "gI", "sI", "D", "m", "gmi", "a", "H") + TIME_TABLES


def host_info(F):
    return {k: v for k, v in F.info().items() if k != "kernel"}  # the kernel is the plan's, made on a GPU


def test_the_case_is_what_the_tests_need():
    c = lr.case()
    sizes = np.bincount(c.labels)
    print(f"unstructured square: {c.mesh.n_elem()} quads, valence-5 vertex {c.star_vertex}, {c.n_domains} subdomains of {sizes.min()} to "
          f"{sizes.max()} elements, mesh grid nt {c.nt_mesh}, coefficient ratios {[int(r) for r in c.ratios]}")
    assert c.mesh.n_elem() == 119 and sizes.max() <= 16 and sizes.min() < 16
    assert set(int(r) for r in c.ratios) == {1, 2, 3}


@pytest.mark.parametrize("precision,real", [("f32", np.float32), ("f64", np.float64)])
def test_rk4_on_coefficient_ratios_host_tables(precision, real):
    c = lr.case()
    F = c.product(precision, integrator="rk4", coarsen=lr.COARSEN, time_ratios="coefficient")
    nt = rk.base_steps(c.nt_mesh, lr.COARSEN)
    assert F.integrator() == ("rk4", lr.COARSEN)
    assert F.info()["nt"] == nt and F.info()["n_domains"] == c.n_domains and F.info()["nel1d"] == 0
    want = tg.coefficient_ratios(c.O["f64"].t, c.h_a)
    assert np.array_equal(F.time_ratios(), want)
    for r in sorted(set(int(v) for v in want)):
        dt, filt, cs, sn = tg.time_grid(c.omega, r * nt, real)
        for name, ref in zip(TIME_TABLES, (filt, cs, sn)):
            got = F.table(f"{name}@{r}")
            assert got.dtype == ref.dtype and got.tobytes() == ref.tobytes(), (name, r)
    with pytest.raises(RuntimeError):
        F.table("filter@4")
    # RK2 with the same ratios stays on the mesh grid
    F2 = c.product(precision, time_ratios="coefficient")
    assert F2.integrator() == ("rk2", 1) and F2.info()["nt"] == c.nt_mesh and np.array_equal(F2.time_ratios(), want)
    dt, filt, cs, sn = tg.time_grid(c.omega, 3 * c.nt_mesh, real)
    assert F2.table("cs@3").tobytes() == cs.tobytes()


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_explicit_ratios_and_a_one_leave_every_table_the_default_plans(precision):
    c = lr.case()
    F0 = c.product(precision)
    assert F0.integrator() == ("rk2", 1) and list(F0.time_ratios()) == [1] * c.n_domains
    explicit = np.arange(c.n_domains, dtype=np.int32) % 3 + 1
    F = c.product(precision, time_ratios=explicit)
    assert np.array_equal(F.time_ratios(), explicit) and host_info(F) == host_info(F0)
    for name in ALL_TABLES:
        assert F.table(name).tobytes() == F0.table(name).tobytes(), name
    for name in TIME_TABLES:
        assert F.table(f"{name}@1").tobytes() == F0.table(name).tobytes(), name
    # a == 1: `coefficient` is the default plan
    G0 = c.product(precision, h_a=c.ones)
    for kw in (dict(time_ratios="coefficient"), dict(time_ratios=None, integrator="rk2", coarsen=1), dict(time_ratios="coefficient", integrator="rk2")):
        G = c.product(precision, h_a=c.ones, **kw)
        assert host_info(G) == host_info(G0) and list(G.time_ratios()) == [1] * c.n_domains
        for name in ALL_TABLES:
            assert G.table(name).tobytes() == G0.table(name).tobytes(), name
    # rk4 at coarsen 1 marches on the mesh grid's tables
    G = c.product(precision, h_a=c.ones, integrator="rk4", coarsen=1)
    assert G.integrator() == ("rk4", 1) and host_info(G) == host_info(G0)
    for name in ALL_TABLES:
        assert G.table(name).tobytes() == G0.table(name).tobytes(), name


def test_refusals_come_before_anything_is_built():
    from cuddhelmholtz_amd import _native as N
    from cuddhelmholtz_amd.api import _h

    c = lr.case()
    nd = c.n_domains
    ones = np.ones(nd, dtype=np.int32)
    for kw in (dict(integrator="rk4", coarsen=0), dict(integrator="rk4", coarsen=17), dict(integrator="rk4", coarsen=2.0),
               dict(integrator="rk2", coarsen=2), dict(integrator="rk3"), dict(integrator=None),
               dict(time_ratios=ones[:-1]), dict(time_ratios=np.ones(nd + 1, dtype=np.int32)), dict(time_ratios=np.zeros(nd, dtype=np.int32)),
               dict(time_ratios=np.full(nd, 257, dtype=np.int32)), dict(time_ratios=np.ones(nd)), dict(time_ratios=ones[:, None]),
               dict(time_ratios="finest"), dict(time_ratios="mesh"),
               dict(time_step="coefficient"), dict(time_step=ones)):
        with pytest.raises(ValueError):
            c.product(**kw)
    for v in (float("nan"), float("inf"), 0.0, -0.4):
        a = c.h_a.copy()
        a[a.size // 2] = v
        with pytest.raises(ValueError):
            c.product(h_a=a, time_ratios="coefficient")
    with pytest.raises(ValueError):
        c.product(h_a=np.full(c.h_a.size, 1 / 257), time_ratios="coefficient")
    assert list(c.product(time_ratios=np.full(nd, 256, dtype=np.int32)).time_ratios()) == [256] * nd
    # the same checks in the C++ constructor, through the C creator, for callers that do not come through Python
    fem = c.fem()
    labels = np.ascontiguousarray(c.labels, dtype=np.int32)

    def create(policy, ratios, scheme, coarsen, h_a=c.h_a, lab=labels):
        r = None if ratios is None else np.asarray(ratios, dtype=np.int32)
        return N.lib.cuddh_ddh_create_labels_integrator(c.omega, _h(np.ascontiguousarray(h_a)), fem._h, nd, _h(lab), 0, 0, policy,
                                                        None if r is None else _h(r), 0 if r is None else r.size, scheme, coarsen)

    for ratios in (ones[:-1], np.r_[ones[:-1], 0], np.r_[ones[:-1], 257]):
        assert not create(2, ratios, 1, 4)
        assert N.last_error().startswith("DDH error: time step"), N.last_error()
    assert not create(3, None, 0, 1) and N.last_error().startswith("DDH error: time step")
    bad_a = c.h_a.copy()
    bad_a[0] = float("nan")
    assert not create(1, None, 0, 1, h_a=bad_a) and N.last_error().startswith("DDH error: time step")
    for scheme, coarsen in ((0, 2), (1, 0), (1, 17), (2, 1), (-1, 1)):
        assert not create(0, None, scheme, coarsen)
        assert N.last_error().startswith("DDH error: integrator"), N.last_error()
    # the order of the checks: the integrator, then the labels, then the time step
    bad_labels = labels.copy()
    bad_labels[0] = nd
    assert not create(2, ones[:-1], 1, 17, lab=bad_labels) and N.last_error().startswith("DDH error: integrator")
    assert not create(2, ones[:-1], 1, 4, lab=bad_labels) and "label" in N.last_error()
    h = create(2, ones, 1, 4)
    assert h
    N.lib.cuddh_ddh_destroy(h)


def test_restatement_in_rk2_mode_is_the_per_subdomain_oracle_on_irregular_labels():
    c = lr.case()
    ref = lr.oracle_outputs("f64")
    got = lr.restated_outputs("rk2", 1, True, "f64")
    e = [rk.rel(a, b) for a, b in zip(got, ref)]
    for nm, x in zip(NAMES, e):
        print(f"[unstructured square, ratios {[int(r) for r in c.ratios]}, rk2 restatement] {nm}: vs per-subdomain fp64 oracle {x:.3e} (gate 1e-13)")
    assert all(np.linalg.norm(r) > 0 for r in ref)
    assert all(x <= 1e-13 for x in e), e
