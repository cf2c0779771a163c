"""CPU: pins tests/lgmres_reference.py (the numpy model the GPU tests of gmres(..., augment=k) are held to), checks what the
augmentation promises on the exact-local-solve trace system, and the parts of the option that need no device: the argument
checks of the Python and C interfaces and the exported symbols."""
import ctypes as C
import functools
import inspect
import pathlib

import numpy as np
import pytest

import cgs2_reference as cr
import lgmres_reference as lr

ROOT = pathlib.Path(__file__).resolve().parent.parent
AUG_ENTRY_POINTS = ("cuddh_gmres_f64_aug", "cuddh_gmres_helmholtz_aug", "cuddh_gmres_ddh_aug", "cuddh_gmres_callback_aug",
                    "cuddh_gmres_callback_sharded_aug")


def dense_system(n=37, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, n)) + 6 * np.eye(n), rng.standard_normal(n)


def bitwise(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("m,maxit,tol", [(5, 8, 1e-10), (40, 3, 1e-9), (7, 30, 1e-6)])
@pytest.mark.parametrize("T", [np.float64, np.float32])
def test_model_without_augmentation_is_the_pinned_gmres(m, maxit, tol, T):
    """k = 0: x, res_norm and the counts of cgs2_reference.gmres_cgs2_ref(..., orth="mgs") bit for bit (test_cgs2_reference.py pins
    that one to oracle.gmres)"""
    A, b = dense_system()
    xr, ir = cr.gmres_cgs2_ref(A, b, m, maxit, tol, T, orth="mgs")
    xl, il = lr.lgmres_ref(A, b, m, maxit, tol, 0, T)
    assert bitwise(xl, xr)
    assert il["res_norm"] == ir["res_norm"]
    assert (il["num_matvec"], il["num_iter"], il["success"]) == (ir["num_matvec"], ir["num_iter"], ir["success"])
    assert not il["pairs"] and all(c[0] == c[1] for c in il["cycles"])


@pytest.mark.parametrize("orth", ["mgs", "cgs2"])
def test_augmented_cycle_minimises_over_the_explicit_columns(orth):
    """k = 3, GMRES(8) on a 37-dof dense system, after every cycle: |r_new| is the least-squares minimum of |r_old - A U y| over
    the cycle's explicit columns U = [v_0 .. v_{m-ka-1}, z_0 .. z_{ka-1}] (numpy.linalg.lstsq) to 1e-10 relative, every stored
    A z equals A @ z to 1e-12, and a cycle with ka pairs applies the operator m - ka times"""
    A, b = dense_system()
    m, k = 8, 3
    _, info = lr.lgmres_ref(A, b, m, 7, 0.0, k, np.float64, orth=orth, record=True)
    assert len(info["history"]) == 6
    for c, h in enumerate(info["history"]):
        ka = min(k, c)
        assert info["cycles"][c] == (m, m - ka) and h["U"].shape == (37, m)
        AU = A @ h["U"]
        y = np.linalg.lstsq(AU, h["r_old"], rcond=None)[0]
        best = np.linalg.norm(h["r_old"] - AU @ y)
        got = np.linalg.norm(h["r_new"])
        assert abs(got - best) <= 1e-10 * best, (c, got, best)
        assert len(h["pairs"]) == min(k, c + 1)
        for z, Az in h["pairs"]:
            assert abs(np.linalg.norm(z) - 1) < 1e-14
            assert np.linalg.norm(Az - A @ z) <= 1e-12 * np.linalg.norm(A @ z)
    assert info["num_matvec"] == 1 + sum(m - min(k, c) + 1 for c in range(6))


def test_model_breakdown_stores_no_pair():
    """A = identity, b = e_1: h[1] == 0 at the first step; the run ends as without augmentation and no pair was stored"""
    b = np.zeros(37)
    b[0] = 1
    for T in (np.float32, np.float64):
        x, info = lr.lgmres_ref(lambda v: v.copy(), b, 5, 10, 1e-6, 2, T)
        assert info["success"] and info["num_matvec"] == 3 and info["res_norm"] == [1.0, 0.0]
        assert np.array_equal(x, b.astype(T)) and not info["pairs"]


def test_model_rejects_a_bad_augment():
    A, b = dense_system()
    for bad in (-1, 5, 6, 1.0, "2"):
        with pytest.raises(ValueError, match="augment"):
            lr.lgmres_ref(A, b, 5, 3, 1e-6, bad)


@functools.lru_cache(maxsize=None)
def trace_runs():
    A, b = lr.trace_system(*lr.TRACE_CASE)
    return A, b, lr.lgmres_ref(A, b, 20, 61, 1e-6, 0), lr.lgmres_ref(A, b, 20, 61, 1e-6, 3)


def test_augmentation_cuts_the_matvecs_on_the_trace_system():
    """trace_system(16, 2, pi) (3,136 real unknowns, 8 x 8 subdomains), tol 1e-6: GMRES(20) and GMRES(20) with k = 3 both succeed
    within 60 cycles and the augmented run needs at most 0.75 x the plain run's matvecs.  The cap is a condition with margin, not
    a measurement: the model measured 313 against 556 (17 against 27 cycles), a ratio of 0.56."""
    A, b, (xp, ip), (xa, ia) = trace_runs()
    assert A.shape == (3136, 3136)
    print(f"GMRES(20): {ip['num_matvec']} matvecs, {ip['num_iter']} cycles; with k = 3: {ia['num_matvec']} matvecs, {ia['num_iter']} cycles")
    assert ip["success"] and ia["success"] and ip["num_iter"] <= 60 and ia["num_iter"] <= 60
    assert ia["num_matvec"] <= 0.75 * ip["num_matvec"]
    for x in (xp, xa):
        assert np.linalg.norm(b - A @ x) < 2e-6 * np.linalg.norm(b)


# ---------------------------------------------------------------- interfaces, no device
class _Stub:
    """stands for an operator: the augment check comes before anything is asked of it"""
    _h = None
    _n = 4


@pytest.mark.parametrize("bad", ["3", 1.0, None, True], ids=repr)
def test_python_rejects_an_augment_of_the_wrong_type(bad):
    import cuddhelmholtz_amd as cd

    with pytest.raises(ValueError, match="augment"):
        cd.gmres(4, None, lambda x, y: None, None, 5, 2, augment=bad)
    with pytest.raises(ValueError, match="augment"):
        cd.HelmholtzOperator.gmres(_Stub(), None, None, 5, 2, augment=bad)


def test_python_rejects_a_negative_augment():
    import cuddhelmholtz_amd as cd

    with pytest.raises(ValueError, match="augment"):
        cd.gmres(4, None, lambda x, y: None, None, 5, 2, augment=-1)
    with pytest.raises(ValueError, match="augment"):
        cd.HelmholtzOperator.gmres(_Stub(), None, None, 5, 2, augment=-1)


def test_python_rejects_an_augment_of_m_or_more():
    import cuddhelmholtz_amd as cd

    for bad in (5, 6, 500):
        with pytest.raises(ValueError, match="augment"):
            cd.gmres(4, None, lambda x, y: None, None, 5, 2, augment=bad)
        with pytest.raises(ValueError, match="augment"):
            cd.HelmholtzOperator.gmres(_Stub(), None, None, 5, 2, augment=bad)
    for f in (cd.gmres, cd.HelmholtzOperator.gmres):
        assert inspect.signature(f).parameters["augment"].default == 0


def test_c_api_rejects_a_bad_augment():
    from cuddhelmholtz_amd import _native as N

    called = []
    cb = N.ACTION_CB(lambda ctx, x, y: called.append(1))
    res = N.SolverResult()
    for bad in (-1, 2, 7):  # m = 2
        rc = N.lib.cuddh_gmres_callback_aug(4, None, cb, None, None, 1, 2, 2, 1e-6, 0, 1.0, 0, bad, C.byref(res), None, None)
        assert rc != 0
        assert N.last_error().startswith("gmres error: augment"), N.last_error()
    rc = N.lib.cuddh_gmres_callback_aug(4, None, cb, None, None, 1, 2, 2, 1e-6, 0, 1.0, 5, 1, C.byref(res), None, None)
    assert rc != 0 and N.last_error().startswith("gmres error: orthogonalization"), N.last_error()
    assert not called


def test_symbols_are_declared_and_exported():
    from cuddhelmholtz_amd import _native as N

    capi = (ROOT / "include" / "cuddh_capi.h").read_text()
    hip = (ROOT / "include" / "cuddh_hip.h").read_text()
    for name in AUG_ENTRY_POINTS:
        assert f"int {name}(" in capi, name
        f = getattr(N.lib, name)
        orth = getattr(N.lib, name[:-4] + "_orth")
        assert len(f.argtypes) == len(orth.argtypes) + 1
    for name in ("cuddh_hip_krylov_update_f64", "cuddh_hip_krylov_update_f32"):
        assert f"int {name}(" in hip, name
        assert len(getattr(N.lib, name).argtypes) == 12
