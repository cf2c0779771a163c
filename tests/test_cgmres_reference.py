"""CPU: tests/cgmres_reference.py (GMRES over the complex numbers on split [Re; Im] vectors in numpy) pinned to the real model,
what complex arithmetic promises on the trace system, and the refusals of the Python and C interfaces that precede any device work."""
import ctypes as C
import functools
import inspect
import pathlib

import numpy as np
import pytest

import cgmres_reference as cg
import lgmres_reference as lr

ROOT = pathlib.Path(__file__).resolve().parent.parent
CPLX_ENTRY_POINTS = ("cuddh_gmres_ddh_cplx", "cuddh_gmres_callback_cplx")
CPLX_KERNELS = ("cuddh_hip_cmgs_ws_bytes", "cuddh_hip_cmgs_stage_f64", "cuddh_hip_cmgs_stage_f32", "cuddh_hip_ckrylov_update_f64",
                "cuddh_hip_ckrylov_update_f32")


def well_conditioned(h, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((h, h)) + 6 * np.eye(h), rng.standard_normal(h)


# ---------------------------------------------------------------- the pin
@pytest.mark.parametrize("m,maxit,tol", [(5, 8, 1e-10), (60, 3, 1e-9), (7, 30, 1e-6)])
@pytest.mark.parametrize("T", [np.float64, np.float32])
@pytest.mark.parametrize("h,seed", [(40, 0), (41, 1)])
def test_model_on_a_real_system_is_the_pinned_real_gmres(h, seed, m, maxit, tol, T):
    """diag(B, B) with right-hand side [b; 0], B and b real: every imaginary quantity is an exact zero and the model reproduces
    lgmres_ref(B, b, m, maxit, tol, 0) bit for bit in x[:h], res_norm and the counts; x[h:] stays zero.  diag(B, B) is applied
    block by block -- B @ v[:h] is then the very product lgmres_ref forms, where one product with the 2 h x 2 h matrix would sum
    each row in another order."""
    B, b = well_conditioned(h, seed)
    Bt = B.astype(T)
    xr, ir = lr.lgmres_ref(B, b, m, maxit, tol, 0, T)
    xc, ic = cg.cgmres_ref(lambda v: np.concatenate([Bt @ v[:h], Bt @ v[h:]]), np.concatenate([b, np.zeros(h)]), m, maxit, tol, T)
    assert xc.dtype == xr.dtype and np.array_equal(xc[:h].view(np.uint8), xr.view(np.uint8))
    assert not np.any(xc[h:])
    assert ic["res_norm"] == ir["res_norm"]
    assert (ic["num_matvec"], ic["num_iter"], ic["success"]) == (ir["num_matvec"], ir["num_iter"], ir["success"])
    assert ic["cycles"] == [c[0] for c in ir["cycles"]]
    assert ir["num_matvec"] > m or ir["success"]


def test_model_breakdown():
    """A = identity, b = e_1: h[1] == 0 at the first step; x = b exactly after one cycle"""
    b = np.zeros(38)
    b[0] = 1
    for T in (np.float32, np.float64):
        x, info = cg.cgmres_ref(lambda v: v.copy(), b, 5, 10, 1e-6, T)
        assert info["success"] and info["num_matvec"] == 3 and info["res_norm"] == [1.0, 0.0]
        assert np.array_equal(x, b.astype(T))


def test_model_rejects_an_odd_length():
    with pytest.raises(ValueError, match="even"):
        cg.cgmres_ref(np.eye(3), np.ones(3), 2, 2, 1e-6)


def test_a_cycle_minimises_over_the_complex_krylov_space():
    """one cycle of m = 6 on a complex-linear system of 30 complex unknowns: |r_1| is the least-squares minimum of |r_0 - K y| over
    COMPLEX y, K the Krylov matrix [r_0, C r_0, ..]: the real iteration's minimum over real y is larger"""
    rng = np.random.default_rng(3)
    h, m = 30, 6
    Cm = 3 * np.eye(h) + (rng.standard_normal((h, h)) + 1j * rng.standard_normal((h, h))) / np.sqrt(h)
    A = np.block([[Cm.real, -Cm.imag], [Cm.imag, Cm.real]])
    c = rng.standard_normal(h) + 1j * rng.standard_normal(h)
    b = np.concatenate([c.real, c.imag])
    _, info = cg.cgmres_ref(A, b, m, 2, 0.0)
    K = np.stack([np.linalg.matrix_power(Cm, j + 1) @ c for j in range(m)], axis=1)
    best = np.linalg.norm(c - K @ np.linalg.lstsq(K, c, rcond=None)[0])
    assert abs(info["res_norm"][1] - best) <= 1e-10 * best
    _, real = lr.lgmres_ref(A, b, m, 2, 0.0, 0)
    assert real["res_norm"][1] > 1.05 * info["res_norm"][1]


# ---------------------------------------------------------------- the trace system
@functools.lru_cache(maxsize=None)
def trace_runs():
    A, b = lr.trace_system(*lr.TRACE_CASE)
    return A, b, lr.lgmres_ref(A, b, 20, 61, 1e-6, 0), cg.cgmres_ref(A, b, 20, 61, 1e-6)


def test_complex_arithmetic_halves_the_matvecs_on_the_trace_system():
    """trace_system(16, 2, pi) (exact local solves: exactly complex-linear; 1,568 complex unknowns), GMRES(20), tol 1e-6: the complex
    model converges on the true residual and needs at most 0.5 x the operator applications of the real model.  Measured when
    this was written: 141 against 551; the cap leaves a factor of two for differences in the exit rule."""
    A, b, (xr, ir), (xc, ic) = trace_runs()
    assert A.shape == (3136, 3136)
    assert cg.complex_linearity_defect(lambda v: A @ v, len(b), np.random.default_rng(0)) < 1e-12
    res = np.linalg.norm(b - A @ xc) / np.linalg.norm(b)
    print(f"GMRES(20) real: {ir['num_matvec']} matvecs, {ir['num_iter']} cycles; complex: {ic['num_matvec']} matvecs, {ic['num_iter']} cycles, "
          f"recomputed relative residual {res:.3e}; |x_c - x_r| / |x_r| = {np.linalg.norm(xc - xr) / np.linalg.norm(xr):.3e}")
    assert ir["success"] and ic["success"]
    assert res < 1e-6
    assert ic["num_matvec"] <= 0.5 * ir["num_matvec"]


def test_an_operator_that_is_not_quite_complex_linear_still_converges():
    """A + 5e-3 |A| R diag(I, -I) on 100 complex unknowns (n = 200): A complex-linear and well conditioned, R random of unit
    2-norm; diag(I, -I) is the conjugation, so the perturbation is antilinear and the operator misses complex linearity at the
    level of the time-stepped DDH.  The in-cycle estimate is then approximate; the model still ends with a true residual below
    tol, recomputed here."""
    rng = np.random.default_rng(11)
    h, tol = 100, 1e-8
    Cm = 3 * np.eye(h) + (rng.standard_normal((h, h)) + 1j * rng.standard_normal((h, h))) / np.sqrt(h)
    A0 = np.block([[Cm.real, -Cm.imag], [Cm.imag, Cm.real]])
    assert np.linalg.cond(A0) < 20
    R = rng.standard_normal((2 * h, 2 * h))
    R /= np.linalg.norm(R, 2)
    A = A0 + 5e-3 * np.linalg.norm(A0, 2) * R @ np.diag(np.concatenate([np.ones(h), -np.ones(h)]))
    defect = cg.complex_linearity_defect(lambda v: A @ v, 2 * h, np.random.default_rng(0))
    assert 1e-4 < defect < 2e-2, defect
    b = rng.standard_normal(2 * h)
    x, info = cg.cgmres_ref(A, b, 20, 50, tol)
    res = np.linalg.norm(b - A @ x) / np.linalg.norm(b)
    print(f"defect {defect:.3e}: {info['num_matvec']} matvecs, {info['num_iter']} cycles, recomputed relative residual {res:.3e}")
    assert info["success"] and res < tol


# ---------------------------------------------------------------- interfaces, no device
def _stub(cls):
    """an instance without a handle: the checks come before anything is asked of it"""
    return object.__new__(cls)


def _gmres(**kw):
    import cuddhelmholtz_amd as cd

    a = dict(n=4, A=lambda x, y: None, m=5)
    a.update(kw)
    n, A, m = a.pop("n"), a.pop("A"), a.pop("m")
    return cd.gmres(n, None, A, None, m, 2, **a)


@pytest.mark.parametrize("bad", ["Complex", "cplx", "", None, 1, True], ids=repr)
def test_python_rejects_another_arithmetic(bad):
    with pytest.raises(ValueError, match="arithmetic"):
        _gmres(arithmetic=bad)


def test_python_rejects_an_odd_length():
    with pytest.raises(ValueError, match="even"):
        _gmres(n=5, arithmetic="complex")


def test_python_rejects_an_operator_handle_or_a_preconditioner():
    import cuddhelmholtz_amd as cd

    with pytest.raises(ValueError, match="complex"):
        _gmres(A=_stub(cd.HelmholtzOperator), arithmetic="complex")
    with pytest.raises(ValueError, match="complex"):
        _gmres(A=_stub(cd.MassMatrix), arithmetic="complex")
    with pytest.raises(ValueError, match="complex"):
        _gmres(Precond=_stub(cd.MassMatrix), arithmetic="complex")
    assert "arithmetic" not in inspect.signature(cd.HelmholtzOperator.gmres).parameters


def test_python_rejects_reduce():
    with pytest.raises(ValueError, match="reduce"):
        _gmres(reduce=lambda t: None, arithmetic="complex")


def test_python_rejects_cgs2_and_augmentation():
    with pytest.raises(ValueError, match="orth"):
        _gmres(orth="cgs2", arithmetic="complex")
    with pytest.raises(ValueError, match="augment"):
        _gmres(augment=2, arithmetic="complex")


def test_real_is_the_default():
    import cuddhelmholtz_amd as cd

    assert inspect.signature(cd.gmres).parameters["arithmetic"].default == "real"


def test_defect_rejects_bad_arguments_before_touching_the_device():
    import cuddhelmholtz_amd as cd

    with pytest.raises(ValueError, match="even"):
        cd.complex_linearity_defect(lambda x, y: None, 5, "f64")
    with pytest.raises(ValueError, match="dtype"):
        cd.complex_linearity_defect(lambda x, y: None, 4, "f16")


def test_c_api_rejects_an_odd_length_and_a_long_restart():
    from cuddhelmholtz_amd import _native as N

    called = []
    cb = N.ACTION_CB(lambda ctx, x, y: called.append(1))
    res = N.SolverResult()
    for n, m in ((5, 2), (4, 513), (4, 0)):
        rc = N.lib.cuddh_gmres_callback_cplx(n, None, cb, None, None, 1, m, 2, 1e-6, 0, 1.0, C.byref(res), None, None)
        assert rc != 0
        assert N.last_error().startswith("gmres error: complex arithmetic"), N.last_error()
    assert not called


def test_symbols_are_declared_and_exported():
    from cuddhelmholtz_amd import _native as N

    capi = (ROOT / "include" / "cuddh_capi.h").read_text()
    hip = (ROOT / "include" / "cuddh_hip.h").read_text()
    for name in CPLX_ENTRY_POINTS:
        assert f"int {name}(" in capi, name
    for name in CPLX_KERNELS:
        assert f" {name}(" in hip, name
    for name in CPLX_ENTRY_POINTS + CPLX_KERNELS:
        assert name in N.declared_symbols() and isinstance(getattr(N.lib, name), C._CFuncPtr)


def test_frozen_longdouble_run_is_the_models():
    """tests/golden/cgmres_trace_longdouble.npz (the model in longdouble on the trace system, what the device test measures the
    float64 model's sensitivity against): the counts are the float64 model's, and the first two cycles recomputed in
    longdouble give the file's first three residual norms to 1e-17 relative (hi + lo carries 106 bits of a longdouble's 64)"""
    g = np.load(cg.golden_path())
    _, _, _, (_, ic) = trace_runs()
    assert int(g["num_matvec"]) == ic["num_matvec"] and g["cycles"].tolist() == ic["cycles"] and len(g["res_hi"]) == len(ic["res_norm"])
    hi, lo, _, _ = cg.trace_longdouble(maxit=3)
    frozen = g["res_hi"][:3].astype(np.longdouble) + g["res_lo"][:3]
    again = hi.astype(np.longdouble) + lo
    assert len(again) == 3 and np.all(np.abs(again - frozen) <= 1e-17 * frozen)
    sens = np.abs(np.asarray(ic["res_norm"]).astype(np.longdouble) - (g["res_hi"].astype(np.longdouble) + g["res_lo"])) / g["res_hi"]
    assert 0 < float(sens.max()) < 1e-9, sens
