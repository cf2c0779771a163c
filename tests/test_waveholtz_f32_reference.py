"""tests/waveholtz_f32_reference.py Model32 against the float64 model, and the refusals of precision="f32": no GPU.

Recorded on the CPU (random z from seed 11, the example load; relative 2-norm of Model32 against waveholtz_reference.Model):
    case ([-1, 1]^2, omega = 2 pi nx / 10)                      nt    period      action
    8 x 8, n_basis 4, rk2                                       800   1.058e-6    7.947e-7
    8 x 8, n_basis 4, rk4 / 4                                   200   1.221e-6    9.443e-7
    8 x 8, n_basis 4, rk4 / 4, smooth a, ratio from it (2)      400   1.438e-6    1.023e-6
    6 x 6, n_basis 5, rk4 / 4                                   313   1.105e-6    6.070e-7
    6 x 6, n_basis 3, rk2                                       451   7.947e-7    4.630e-7
    16 x 16, n_basis 4, rk4 / 4                                 200   1.215e-6    1.130e-6
The test holds the model to the two-digit figures these were published with (TABLE), to 1 % of each: numpy's elementwise float32
operations and scipy's row-by-row matrix product are the same operations in the same order everywhere.

GMRES(20) on the 8 x 8 rk4 / 4 case: 11 / 12 / 13 matvecs at tol 2e-4 / 1e-4 / 5e-5 on both models; the per-step estimates around the
stop at 1e-4 are 1.92e-4, 5.6e-5 and 1.6e-5 of |b|, so 1e-4 sits a factor 1.8 - 1.9 from both neighbours.
"""
import functools

import numpy as np
import pytest

import cuddhelmholtz_amd as cd
import waveholtz_f32_reference as w32
import waveholtz_reference as wr
from cuddhelmholtz_amd import _native as N

# (nx, n_basis, smooth a, scheme, coarsen, time_ratio): nt, period and action error to two digits
TABLE = {
    (8, 4, False, "rk2", 1, 1): (800, 1.06e-6, 7.9e-7),
    (8, 4, False, "rk4", 4, 1): (200, 1.22e-6, 9.4e-7),
    (8, 4, True, "rk4", 4, "coefficient"): (400, 1.44e-6, 1.02e-6),
    (6, 5, False, "rk4", 4, 1): (313, 1.11e-6, 6.1e-7),
    (6, 3, False, "rk2", 1, 1): (451, 7.9e-7, 4.6e-7),
    (16, 4, False, "rk4", 4, 1): (200, 1.22e-6, 1.13e-6),
}


@functools.lru_cache(maxsize=None)
def models(nx, nb, smooth, scheme, coarsen, time_ratio):
    c = wr.uniform_case(nx, nb, smooth)
    ratio = wr.coefficient_ratio(c.h_a) if time_ratio == "coefficient" else time_ratio
    M = c.model(scheme, coarsen, ratio, "lobatto")
    return c, M, w32.Model32.of(M)


@pytest.mark.parametrize("case", list(TABLE), ids=lambda c: f"{c[0]}x{c[0]}-nb{c[1]}-{c[3]}" + ("-smooth" if c[2] else ""))
def test_model32_reproduces_the_recorded_errors(case):
    nt, want_period, want_action = TABLE[case]
    c, M, M32 = models(*case)
    assert M.nt == M32.nt == nt
    z = np.random.default_rng(11).standard_normal(2 * M.n)
    got, got_action = M32.period(z, c.f), M32.action(z)
    assert got.dtype == got_action.dtype == np.float64
    err, err_action = wr.rel(got, M.period(z, c.f)), wr.rel(got_action, M.action(z))
    print(f"Model32 against Model {case}: nt={nt} period {err:.3e} action {err_action:.3e}")
    assert abs(err / want_period - 1.0) < 0.01 and abs(err_action / want_action - 1.0) < 0.01
    # the absent arguments of the float64 model
    assert np.array_equal(M32.period(None, c.f), M32.period(np.zeros(2 * M.n), c.f))
    assert np.array_equal(M32.period(z, None), M32.period(z, np.zeros(2 * M.n)))


def test_gmres_counts_do_not_see_the_precision_at_1e_4():
    c, M, M32 = models(8, 4, False, "rk4", 4, 1)
    for tol, matvecs in ((2e-4, 11), (1e-4, 12), (5e-5, 13)):
        for model in (M, M32):
            z, info = model.gmres(c.f, 20, 100, tol)
            assert info["success"] and info["num_matvec"] == matvecs, (tol, type(model).__name__, info["num_matvec"])
            if tol == 1e-4:
                b = M.rhs(c.f)  # the residual of either solution in the float64 operator
                res = float(np.linalg.norm(b - M.action(z)) / np.linalg.norm(b))
                print(f"GMRES(20) tol 1e-4 on {type(model).__name__}: {info['num_matvec']} matvecs, float64 residual {res / tol:.3f} tol")
                assert res < tol


class NoSpace:  # anything that touches the space fails the test with another exception
    def __getattr__(self, name):
        raise AssertionError(f"the space was used ({name}) before the arguments were checked")


@pytest.mark.parametrize("kwargs", [dict(precision="f16", stiffness="lobatto", sweep="lattice"), dict(precision=1, stiffness="lobatto", sweep="lattice"),
                                    dict(precision="f32", sweep="operator"), dict(precision="f32", stiffness="lobatto"), dict(precision="f32")],
                         ids=["f16", "1", "f32-operator", "f32-lobatto-operator", "f32-default-sweep"])
def test_bad_precision_raises_before_the_space_is_touched(kwargs):
    with pytest.raises(ValueError, match="precision"):
        cd.WaveHoltz(1.0, np.ones(4), NoSpace(), **kwargs)


def test_precisions_are_named():
    assert cd.WaveHoltz.PRECISIONS == ("f64", "f32")


def test_native_refusals_of_the_precision():
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(2, -1.0, 1.0, 2, -1.0, 1.0), cd.Basis(2))
    a = np.ones(fem.size())
    for stiffness, sweep, precision in ((1, 0, 1), (0, 0, 1), (1, 1, 2), (1, 1, -1), (1, 0, 2)):
        h = N.lib.cuddh_waveholtz_create_precision(1.0, a.ctypes.data, fem._h, 0, 1, 1, stiffness, None, -1, sweep, precision)
        assert not h and N.last_error().startswith("WaveHoltz error: precision:"), (stiffness, sweep, precision, N.last_error())
    # the sweep's own refusals come through unchanged
    h = N.lib.cuddh_waveholtz_create_precision(1.0, a.ctypes.data, fem._h, 0, 1, 1, 0, None, -1, 1, 0)
    assert not h and N.last_error().startswith("WaveHoltz error: sweep:"), N.last_error()
    assert N.lib.cuddh_waveholtz_precision(None) == -1
