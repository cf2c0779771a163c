"""The small problem of a GMRES(m) cycle (csrc/src/gmres_small.hpp: Givens rotations of the Hessenberg columns, residual estimate,
back substitution) through cuddh_gmres_small_problem, as krylov.cpp compiles it.  Host code: no GPU.  Reference: numpy.linalg.lstsq on
the (ncols + 1) x ncols Hessenberg system min |beta e_1 - H y|.

Bound: a backward-stable solution of a least-squares problem with a residual of the size of the right-hand side is off by a modest
multiple of eps cond(H) (here cond(H) <= 10, asserted, so cond^2 terms stay below it); ncols <= m rotations and one triangular
solve give the factor m, and 100 covers the constants: 100 m eps cond(H), relative.  eps is that of the entries: float32 for "f32",
float64 otherwise (complex entries are held in double on the host whatever the vectors' type)."""
import ctypes as C

import numpy as np
import pytest

from cuddhelmholtz_amd import _native as N

lib = N.lib
BETA = 1.75
KINDS = {"f64": (0, 1, np.float64), "f32": (0, 0, np.float32), "complex": (1, 1, np.float64)}  # is_complex, is_f64, stored type
SHAPES = [(m, ncols) for m in (1, 2, 5) for ncols in sorted({1, m})]


def hessenberg(kind, m, ncols, seed=0):
    """(ncols + 1) x ncols, upper Hessenberg with a positive real subdiagonal, entries exactly representable in the stored type;
    a dominant diagonal keeps cond(H) <= 10 (asserted by the callers)"""
    rng = np.random.default_rng(1000 * seed + 10 * m + ncols)
    stored = KINDS[kind][2]

    def entries(*shape):
        re = rng.uniform(-0.4, 0.4, shape).astype(stored).astype(np.float64)
        if kind != "complex":
            return re
        return re + 1j * rng.uniform(-0.4, 0.4, shape).astype(stored).astype(np.float64)

    H = np.zeros((ncols + 1, ncols), dtype=np.complex128 if kind == "complex" else np.float64)
    H[:ncols, :] = np.triu(entries(ncols, ncols), 1)
    phase = entries(ncols)
    phase = np.where(phase == 0, 1.0, phase)
    H[np.arange(ncols), np.arange(ncols)] = (phase / np.abs(phase) * rng.uniform(1.0, 1.5, ncols)).astype(H.dtype)
    H[np.arange(1, ncols + 1), np.arange(ncols)] = rng.uniform(0.2, 0.6, ncols)
    if kind == "f32":
        H = H.astype(np.float32).astype(np.float64)
    return H


def pack(H, kind):
    """column k as k + 2 entries, one column after another; re, im interleaved when complex"""
    flat = np.concatenate([H[:k + 2, k] for k in range(H.shape[1])])
    if kind == "complex":
        return np.ascontiguousarray(np.stack([flat.real, flat.imag], axis=1).reshape(-1))
    return np.ascontiguousarray(flat.astype(KINDS[kind][2]))


def run(H, kind, m):
    """(y, est) of the library"""
    is_complex, is_f64, stored = KINDS[kind]
    ncols = H.shape[1]
    cols = pack(H, kind)
    y = np.full(ncols * (2 if is_complex else 1), np.nan, dtype=stored)
    est = np.full(ncols, np.nan)
    rc = lib.cuddh_gmres_small_problem(is_complex, is_f64, m, ncols, cols.ctypes.data_as(C.c_void_p), BETA, y.ctypes.data_as(C.c_void_p),
                                       est.ctypes.data_as(C.c_void_p))
    assert rc == 0, N.last_error()
    if is_complex:
        y = y[0::2] + 1j * y[1::2]
    return y.astype(np.complex128 if is_complex else np.float64), est


def reference(H):
    rhs = np.zeros(H.shape[0], dtype=H.dtype)
    rhs[0] = BETA
    y = np.linalg.lstsq(H, rhs, rcond=None)[0]
    return y, float(np.linalg.norm(rhs - H @ y))


def bound(H, kind, m):
    cond = float(np.linalg.cond(H))
    assert cond <= 10, (kind, H.shape, cond)
    return 100 * m * float(np.finfo(KINDS[kind][2]).eps) * cond


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("m,ncols", SHAPES)
def test_small_problem_against_lstsq(kind, m, ncols):
    H = hessenberg(kind, m, ncols)
    tol = bound(H, kind, m)
    y, est = run(H, kind, m)
    y_ref, res_ref = reference(H)
    err_y = float(np.linalg.norm(y - y_ref) / np.linalg.norm(y_ref))
    err_est = abs(est[ncols - 1] - res_ref) / res_ref
    print(f"{kind} m={m} ncols={ncols}: cond {np.linalg.cond(H):.3f}, |y - y_ref| / |y_ref| = {err_y:.3e}, estimate off by {err_est:.3e}, bound {tol:.3e}")
    assert err_y <= tol
    assert err_est <= tol
    # the estimate after each column is the residual of the leading problem: it cannot grow
    assert np.all(np.isfinite(est)) and np.all(np.diff(est) <= tol * BETA) and est[0] <= BETA * (1 + tol)


@pytest.mark.parametrize("m,ncols", SHAPES)
def test_complex_with_real_entries_is_the_real_path(m, ncols):
    H = hessenberg("f64", m, ncols)
    tol = bound(H, "f64", m)
    y_real, est_real = run(H, "f64", m)
    y_cplx, est_cplx = run(H.astype(np.complex128), "complex", m)
    assert np.linalg.norm(y_cplx - y_real) <= tol * np.linalg.norm(y_real)
    assert np.all(np.abs(est_cplx - est_real) <= tol * est_real)


def test_bad_arguments_are_refused_and_write_nothing():
    H = hessenberg("f64", 2, 2)
    cols = pack(H, "f64")
    y = np.full(2, -7.0)
    est = np.full(2, -7.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for args in ((0, 1, 0, 1, p(cols), BETA, p(y), p(est)),   # m < 1
                 (0, 1, 2, 3, p(cols), BETA, p(y), p(est)),   # ncols > m
                 (1, 1, 2, 3, p(cols), BETA, p(y), p(est)),
                 (0, 1, 2, 2, None, BETA, p(y), p(est)),
                 (0, 1, 2, 2, p(cols), BETA, None, p(est)),
                 (0, 1, 2, 2, p(cols), BETA, p(y), None)):
        assert lib.cuddh_gmres_small_problem(*args) != 0, args
        assert N.last_error().startswith("gmres small problem"), N.last_error()
        assert np.all(y == -7.0) and np.all(est == -7.0)


def test_symbol_is_declared_and_exported():
    from pathlib import Path

    capi = (Path(__file__).resolve().parents[1] / "include" / "cuddh_capi.h").read_text()
    assert "int cuddh_gmres_small_problem(" in capi
    assert "cuddh_gmres_small_problem" in N.declared_symbols() and isinstance(lib.cuddh_gmres_small_problem, C._CFuncPtr)
