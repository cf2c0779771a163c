"""CPU: pins tests/cgs2_reference.py (the numpy model the GPU tests of the CGS2 option are held to) and the parts of the option
that need no device: the argument checks of the Python and C interfaces and the exported symbols."""
import ctypes as C
import pathlib

import numpy as np
import pytest

import blas1_reference as br
import cgs2_reference as cr
import oracle

ROOT = pathlib.Path(__file__).resolve().parent.parent
ORTH_ENTRY_POINTS = ("cuddh_gmres_f64_orth", "cuddh_gmres_helmholtz_orth", "cuddh_gmres_ddh_orth", "cuddh_gmres_callback_orth",
                     "cuddh_gmres_callback_sharded_orth")
CGS_ENTRY_POINTS = ("cuddh_hip_cgs_pass_f64", "cuddh_hip_cgs_pass_f32", "cuddh_hip_cgs_reduce_f64", "cuddh_hip_cgs_reduce_f32",
                    "cuddh_hip_cgs_ws_bytes", "cuddh_hip_cgs_partials")


def dense_system(n=37, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, n)) + 6 * np.eye(n), rng.standard_normal(n)


@pytest.mark.parametrize("m,maxit,tol", [(5, 8, 1e-10), (40, 3, 1e-9), (7, 30, 1e-6)])
def test_helper_with_mgs_is_oracle_gmres(m, maxit, tol):
    """the helper's iteration logic (cycle count, exit tests, num_matvec, res_norm) is the oracle's: with the orthogonalisation
    switched to modified Gram-Schmidt it reproduces oracle.gmres on a 37-dof dense system"""
    A, b = dense_system()
    xo, io = oracle.gmres(lambda v: A @ v, b, m=m, maxit=maxit, tol=tol)
    xh, ih = cr.gmres_cgs2_ref(A, b, m, maxit, tol, np.float64, orth="mgs")
    assert ih["num_matvec"] == io["num_matvec"] and ih["num_iter"] == io["num_iter"] and ih["success"] == io["success"]
    assert len(ih["res_norm"]) == len(io["res_norm"])
    assert np.allclose(ih["res_norm"], io["res_norm"], rtol=1e-13, atol=0)
    assert np.allclose(xh, xo, rtol=1e-12, atol=0)


def test_helper_with_cgs2_converges_like_mgs():
    """same Krylov spaces: on a well-conditioned system the two orthogonalisations stop at the same step"""
    A, b = dense_system()
    _, im = cr.gmres_cgs2_ref(A, b, 40, 3, 1e-9, np.float64, orth="mgs")
    xc, ic = cr.gmres_cgs2_ref(A, b, 40, 3, 1e-9, np.float64)
    assert ic["success"] and ic["num_matvec"] == im["num_matvec"]
    assert np.linalg.norm(b - A @ xc) < 1e-8 * np.linalg.norm(b)


def test_helper_breakdown():
    """A = identity, b = e_1: h[1] == 0 exactly, as the callback-path breakdown test expects of the device"""
    b = np.zeros(37)
    b[0] = 1
    for T in (np.float32, np.float64):
        x, info = cr.gmres_cgs2_ref(lambda v: v.copy(), b, 5, 10, 1e-6, T)
        assert info["success"] and info["num_matvec"] == 3 and info["res_norm"] == [1.0, 0.0]
        assert np.array_equal(x, b.astype(T))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_orthogonality_separation(dtype):
    """20 Arnoldi steps on diag(geomspace(1, 1e6, 300)) in the working precision: the CGS2 basis is orthogonal to 2 eps, the basis
    of the chain krylov.cpp queues by default (br.mgs_chain_ref) loses more than 20 eps.  Measured here: 1.2 eps (f32) and 1.6 eps
    (f64) against 41 eps in either precision.  tests/test_gpu_cgs2_kernels.py relies on this separation."""
    diag, b, steps = cr.separation_case()
    eps = float(np.finfo(br.NP[dtype]).eps)
    cgs2 = cr.orthogonality_loss(cr.arnoldi_basis(diag, b, steps, dtype, "cgs2"), dtype)
    mgs = cr.orthogonality_loss(cr.arnoldi_basis(diag, b, steps, dtype, "mgs"), dtype)
    print(f"{dtype}: max|V^T V - I| = {cgs2 / eps:.2f} eps (cgs2), {mgs / eps:.2f} eps (mgs)")
    assert cgs2 <= 2 * eps
    assert mgs > 20 * eps


def test_step_in_wide_precision_is_orthogonal_to_the_basis():
    rng = np.random.default_rng(3)
    V = br.orthonormal_columns(200, 5, rng, "f64")
    h, q, c1 = cr.cgs_step_ref(rng.standard_normal(200), V, dtype="f64")
    assert q.dtype == br.wide("f64") and len(h) == 6 and len(c1) == 5
    assert max(abs(float(np.dot(q, v.astype(q.dtype)))) for v in V) < 4 * np.finfo(np.float64).eps


def test_exact_case_stays_exact():
    """the integer case of the kernel test: every sum below the exactness limit at every size and k1 it is used with, disjoint
    supports, and at the ragged size every basis vector nonzero"""
    for dtype in ("f64", "f32"):
        s = br.sizes(dtype)
        for n in s["small"] + s["tile"] + s["ragged"]:
            for k1 in (1, 2, cr.KC, cr.KC + 1, 2 * cr.KC + 1) + ((33,) if n in s["ragged"] else ()):
                w, V = cr.exact_cgs(n, dtype, k1, np.random.default_rng(n))
                assert cr.exact_step(w, V)["largest"] <= br.EXACT_LIMIT[dtype] // 4
                assert np.all(sum(np.abs(v) for v in V) <= 1)
                if n in s["ragged"]:
                    assert all(v.any() for v in V)


# ---------------------------------------------------------------- interfaces, no device
class _Stub:
    """stands for an operator: the orth check comes before anything is asked of it"""
    _h = None
    _n = 4


def test_python_rejects_an_unknown_orthogonalisation():
    import cuddhelmholtz_amd as cd

    for bad in ("bogus", "CGS2", "", None, 1):
        with pytest.raises(ValueError, match="orth"):
            cd.gmres(4, None, lambda x, y: None, None, 2, 2, orth=bad)
        with pytest.raises(ValueError, match="orth"):
            cd.HelmholtzOperator.gmres(_Stub(), None, None, 2, 2, orth=bad)
    import inspect

    for f in (cd.gmres, cd.HelmholtzOperator.gmres):
        assert inspect.signature(f).parameters["orth"].default == "mgs"


def test_c_api_rejects_an_unknown_orthogonalisation():
    from cuddhelmholtz_amd import _native as N

    called = []
    cb = N.ACTION_CB(lambda ctx, x, y: called.append(1))
    res = N.SolverResult()
    for bad in (7, -1, 2):
        rc = N.lib.cuddh_gmres_callback_orth(4, None, cb, None, None, 1, 2, 2, 1e-6, 0, 1.0, bad, C.byref(res), None, None)
        assert rc != 0
        assert N.last_error().startswith("gmres error: orthogonalization"), N.last_error()
    assert not called


def test_symbols_are_declared_and_exported():
    from cuddhelmholtz_amd import _native as N

    capi = (ROOT / "include" / "cuddh_capi.h").read_text()
    hip = (ROOT / "include" / "cuddh_hip.h").read_text()
    for name in ORTH_ENTRY_POINTS:
        assert f"int {name}(" in capi, name
        f = getattr(N.lib, name)
        assert f.argtypes is not None and C.c_int in f.argtypes
    for name in CGS_ENTRY_POINTS:
        assert f" {name}(" in hip, name
        assert getattr(N.lib, name).argtypes is not None
    assert N.lib.cuddh_hip_cgs_ws_bytes(20) == 21 * cr.ROW * 8
    assert N.lib.cuddh_hip_cgs_ws_bytes(0) == cr.ROW * 8
    assert N.lib.cuddh_hip_cgs_partials(0) == 1 and N.lib.cuddh_hip_cgs_partials(10 ** 8) == br.MAX_PARTIALS
    for n in (1, 2047, 2048, 2049, 12311):
        assert N.lib.cuddh_hip_cgs_partials(n) == br.mgs_grid(n)
