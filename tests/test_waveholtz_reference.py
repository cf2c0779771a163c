"""tests/waveholtz_reference.py, the numpy model of the whole-domain WaveHoltz march, pinned before the GPU tests rely on it; and
the argument checks of cd.WaveHoltz, which need no device.

(a) With the collocated K, five periods from zero are what DDH's local solve does on one subdomain that covers the mesh:
    equal to ddh_rk.Restatement.postprocess on those tables to 1e-13 (measured 6e-16 rk2, 4e-16 rk4/4 at 8 x 8).
(b) The model's fixed point (lgmres_ref, k = 0, GMRES(20), tol 1e-8) lies within the time error of the direct solve of
    (K - w^2 M + i w H) U = f.  Recorded distances: 4.87e-5 for rk2 at 8 x 8 (the midpoint rule's time error) and 7.41e-8 for
    rk4 / coarsen 4 at 16 x 16, in 20 and 39 matvecs; gated at twice those.
(c) The Gauss-Legendre K built column by column from the oracle's apply is symmetric and annihilates constants to 1e-12.
"""
import math

import numpy as np
import pytest

import ddh_rk
import waveholtz_reference as wr

RECORDED_DISTANCE = {("rk2", 1, 8): 4.87e-5, ("rk4", 4, 16): 7.42e-8}
RECORDED_MATVECS = {("rk2", 1, 8): 20, ("rk4", 4, 16): 39}


@pytest.mark.parametrize("scheme,coarsen", [("rk2", 1), ("rk4", 4)])
def test_five_periods_are_the_one_subdomain_local_solve(scheme, coarsen):
    c = wr.uniform_case(8, 4)
    assert math.isclose(c.omega, 1.6 * math.pi)
    M = c.model(scheme, coarsen, 1, "lobatto")
    R = ddh_rk.Restatement(c.O, scheme, None, coarsen)
    assert M.nt == R.nt_base == (800 if scheme == "rk2" else 200)
    ref = R.postprocess(np.zeros(c.O.size), c.f)
    err = wr.rel(M.solution(M.iterate(c.f, 5)), ref)
    print(f"{scheme}/{coarsen}: five periods vs Restatement.postprocess {err:.2e}")
    assert err < 1e-13


def test_lumped_matrices_are_the_tables():
    c = wr.uniform_case(8, 4)
    for mine, theirs in zip(c.mh, c.mh_tables):
        assert np.array_equal(mine, theirs)
    assert np.count_nonzero(c.mh[1]) == 4 * 8 * 3  # every boundary dof and no other


@pytest.mark.parametrize("scheme,coarsen,nx", list(RECORDED_DISTANCE))
def test_fixed_point_is_the_direct_solve_up_to_the_time_error(scheme, coarsen, nx):
    c = wr.uniform_case(nx, 4)
    M = c.model(scheme, coarsen, 1, "lobatto")
    z, info = M.gmres(c.f, 20, 100, 1e-8)
    dist = wr.rel(M.solution(z), M.direct(c.f))
    print(f"{scheme}/{coarsen} at {nx} x {nx}: {info['num_matvec']} matvecs, distance to the direct solve {dist:.3e}")
    assert info["success"] and info["num_matvec"] == RECORDED_MATVECS[scheme, coarsen, nx]
    assert dist < 2 * RECORDED_DISTANCE[scheme, coarsen, nx]
    # affine: W(z; f) = S z + W(0; f), which is what makes (I - S) z = W(0; f) the fixed point's equation
    x = np.random.default_rng(3).standard_normal(2 * M.n)
    assert wr.rel(M.period(x, c.f), M.period(x, None) + M.rhs(c.f)) < 1e-13


@pytest.mark.parametrize("nx,nb", [(8, 4), (6, 3), (6, 5)])
def test_gauss_stiffness_is_symmetric_and_annihilates_constants(nx, nb):
    K = wr.uniform_case(nx, nb).K_gauss
    scale = np.abs(K).max()
    assert np.abs(K - K.T).max() < 1e-12 * scale
    assert np.abs(K @ np.ones(K.shape[0])).max() < 1e-12 * scale
    assert np.all(np.linalg.eigvalsh(K) > -1e-10 * scale)


def test_gauss_stiffness_on_the_unstructured_square(unstructured_square):
    import oracle

    xy, elems = unstructured_square
    K = wr.gauss_stiffness(oracle.Discretization(oracle.Mesh(xy, elems), 4))
    scale = np.abs(K).max()
    assert np.abs(K - K.T).max() < 1e-12 * scale and np.abs(K @ np.ones(K.shape[0])).max() < 1e-12 * scale


def test_step_counts_and_the_coefficient_ratio():
    c = wr.uniform_case(8, 4)
    assert (c.nt(), c.nt(4), c.nt(1, 2), c.nt(4, 3)) == (800, 200, 1600, 600)
    assert wr.coefficient_ratio(np.array([1.0, 0.6])) == 2 and wr.coefficient_ratio(np.array([0.2, 1.0])) == 5
    assert wr.coefficient_ratio(np.array([1.0, 3.0])) == 1
    a = wr.smooth_coefficient(c.d)
    assert 0.6 <= a.min() < 0.65 and 0.95 < a.max() <= 1.0


# ---- the Python interface: every bad argument is a ValueError before any native call (fem is never looked at)
def test_waveholtz_is_exported():
    import cuddhelmholtz_amd as cd

    assert "WaveHoltz" in cd.__all__ and issubclass(cd.WaveHoltz, cd.api._Operator)


@pytest.mark.parametrize("kwargs,word", [
    (dict(integrator="rk3"), "integrator"),
    (dict(integrator=4), "integrator"),
    (dict(integrator="rk4", coarsen=0), "coarsen"),
    (dict(integrator="rk4", coarsen=17), "coarsen"),
    (dict(integrator="rk4", coarsen=2.0), "coarsen"),
    (dict(integrator="rk4", coarsen=True), "coarsen"),
    (dict(integrator="rk2", coarsen=2), "rk2"),
    (dict(time_ratio=0), "time_ratio"),
    (dict(time_ratio=257), "time_ratio"),
    (dict(time_ratio=1.5), "time_ratio"),
    (dict(time_ratio="mesh"), "time_ratio"),
    (dict(time_ratio=True), "time_ratio"),
    (dict(stiffness="lumped"), "stiffness"),
    (dict(stiffness=1), "stiffness"),
    (dict(faces=[[1, 2]]), "faces"),
    (dict(faces=[0.5]), "faces"),
])
def test_bad_arguments_raise_before_any_native_call(kwargs, word):
    import cuddhelmholtz_amd as cd

    class NoSpace:  # anything that touches the space fails the test with another exception
        def __getattr__(self, name):
            raise AssertionError(f"the space was used ({name}) before the arguments were checked")

    with pytest.raises(ValueError, match=word):
        cd.WaveHoltz(1.0, np.ones(4), NoSpace(), **kwargs)


def test_bad_coefficient_and_native_refusals_raise_value_errors():
    """no device needed: the space and its tables are host-side, and the constructor refuses before it allocates"""
    import cuddhelmholtz_amd as cd
    from cuddhelmholtz_amd import _native as N

    fem = cd.H1Space(cd.Mesh2D.uniform_rect(2, -1.0, 1.0, 2, -1.0, 1.0), cd.Basis(2))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        a = np.ones(fem.size())
        a[3] = bad
        with pytest.raises(ValueError, match="finite and positive"):
            cd.WaveHoltz(1.0, a, fem)
    with pytest.raises(ValueError, match="coefficient values"):
        cd.WaveHoltz(1.0, np.ones(fem.size() + 1), fem)
    # the C API refuses the same things by itself
    good, bad = np.ones(fem.size()), np.ones(fem.size())
    bad[0] = -2.0
    for args in ((0, 2, 1, 0), (1, 17, 1, 0), (2, 1, 1, 0), (0, 1, 300, 0), (0, 1, 1, 2), (0, 1, 1, 0)):
        a = bad if args == (0, 1, 1, 0) else good
        h = N.lib.cuddh_waveholtz_create(1.0, a.ctypes.data, fem._h, *args, None, -1)
        assert not h and N.last_error().startswith("WaveHoltz error"), (args, N.last_error())
