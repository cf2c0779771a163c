"""Restarted GMRES over the complex numbers on split [Re; Im] vectors, restated in numpy (TEST INFRASTRUCTURE, not collected).

Shared by tests/test_cgmres_reference.py (CPU: pins `cgmres_ref` to lgmres_reference.lgmres_ref with k = 0, which is pinned to
cgs2_reference.gmres_cgs2_ref and through it to oracle.gmres, and checks what complex arithmetic promises) and
tests/test_gpu_gmres_complex.py (gmres(..., arithmetic="complex") on the device).

The iteration (krylov.cpp under ComplexArithmetic): a vector of n = 2 h entries stands for h complex numbers, real parts at
[0, h), imaginary parts at [h, 2 h).  Inner products are <v, w> = sum conj(v) w = (v_r.w_r + v_i.w_i) + i (v_r.w_i - v_i.w_r);
modified Gram-Schmidt with complex coefficients, w <- w - c v; the norm is the real norm of the 2 h entries and the
normalisation a real scaling.  Complex Hessenberg matrix; rotations G_j = [conj(cs_j), conj(sn_j); -sn_j, cs_j] with
cs_j = h_j / t, sn_j = h_{j+1} / t, t = sqrt(|h_j|^2 + |h_{j+1}|^2); inner exit when |eta_{j+1}| < tol |b|, breakdown when
h_{j+1} == 0, as in lgmres_ref.  End of cycle: x <- x + y_j v_j in ascending j, the true residual b - A x, and the decision on it.

Every operation is carried out in the working precision `T` on real and imaginary parts held apart (so that T may be
np.float32 or np.longdouble), each complex product as (a_r b_r - a_i b_i) + i (a_r b_i + a_i b_r) and each quotient by
Smith's formula.  With every imaginary part an exact zero these are the operations of lgmres_ref, one for one: that is the pin.
Inner products are taken per half (np.dot over h entries each), as lgmres_ref takes its own over the h entries of the real
system; the order of the partial sums is otherwise numpy's.
"""
from __future__ import annotations

import numpy as np

import blas1_reference as br

# ---- constants of the complex kernels of kernels/blas1.hip (cmgs_stage_kernel, ckrylov_update_kernel)
CUNROLL = br.UNROLL // 2  # 16-byte accesses of a thread per tile and half
CTILE = CUNROLL * br.BLOCK  # 16-byte vectors of ONE half per tile: 512
CPLX_ROW = br.MAX_PARTIALS  # distance of the real and the imaginary row of partial sums
KMAX = 512  # largest k1 of one update launch (CGS_KMAX)


def cplx_grid(h: int) -> int:
    """workgroups of a complex stage or update on h complex numbers: those of the real chain on the same 2 h scalars"""
    return br.mgs_grid(2 * h)


def sizes(dtype: str) -> dict:
    """size group -> numbers h of complex entries: every h at which the complex kernels take another path.  16-byte accesses need
    h to be a multiple of the vector width N; every other h takes the element-wise path for the whole vector."""
    N = br.PACK[dtype]
    item = np.dtype(br.NP[dtype]).itemsize
    nt = br.NT_BYTES // (2 * item)  # 2 h scalars reach the non-temporal threshold of the update
    return {
        "small": [1, 2, 3, 63, 64, 65, 255, 257],
        "tile": sorted({CTILE * N - 1, CTILE * N, CTILE * N + 1, br.TILE - 1, br.TILE, br.TILE + 1, 2 * CTILE * N - 1, 2 * CTILE * N, 2 * CTILE * N + 1}),
        "ragged": [3 * CTILE * N + 5 * N, 3 * CTILE * N + 5 * N + 1],
        "further": [N * (CTILE * br.MAX_PARTIALS + 300)],  # more than MAX_PARTIALS tiles: a workgroup's second tile
        "nt": [nt - 1, nt, nt + 1],
    }


def marked(h: int, dtype: str) -> list:
    """indices in [0, h) where a clamped load, a tail loop or a tile loop goes wrong (blas1_reference.marked for one half)"""
    N = br.PACK[dtype]
    nv = h // N if h % N == 0 else 0
    places = [0, CTILE * N - 1, CTILE * N, N * CTILE * br.MAX_PARTIALS + 3, h - 1] + list(range((nv - 1) * N, nv * N))
    return sorted({i for i in places if 0 <= i < h})


def times_i(x):
    """i [a; b] = [-b; a]"""
    h = len(x) // 2
    return np.concatenate([-x[h:], x[:h]])


def complex_linearity_defect(apply, n, rng):
    """|A(i x) - i A(x)| / |A x| on one standard normal x"""
    x = rng.standard_normal(n)
    y = np.asarray(apply(x))
    return float(np.linalg.norm(np.asarray(apply(times_i(x))) - times_i(y)) / np.linalg.norm(y))


def cgmres_ref(A, b, m, maxit, tol, T=np.float64, x0=None):
    """A: a real (2 h x 2 h) matrix or a callable x -> A x on split vectors.  Returns (x, info); info as lgmres_ref's
    (success, num_matvec, res_norm, res_norm_unrounded, num_iter, cycles: columns per cycle)."""
    apply = (lambda v: A @ v) if isinstance(A, np.ndarray) else A
    if isinstance(A, np.ndarray):
        A = A.astype(T)
    n = len(b)
    if n % 2:
        raise ValueError(f"split vectors have an even length, not {n}")
    h = n // 2
    b = np.asarray(b, dtype=T)
    x = np.zeros(n, dtype=T) if x0 is None else np.array(x0, dtype=T)
    one = T(1)

    def dot(u, v):
        return T(np.dot(u, v))

    def nrm(v):
        return T(np.sqrt(dot(v[:h], v[:h]) + dot(v[h:], v[h:])))

    def cmul(a, c):
        return (a[0] * c[0] - a[1] * c[1], a[0] * c[1] + a[1] * c[0])

    def cdiv(a, c):
        if abs(c[0]) >= abs(c[1]):
            q = c[1] / c[0]
            d = c[0] + c[1] * q
            return ((a[0] + a[1] * q) / d, (a[1] - a[0] * q) / d)
        q = c[0] / c[1]
        d = c[0] * q + c[1]
        return ((a[0] * q + a[1]) / d, (a[1] * q - a[0]) / d)

    def conj(a):
        return (a[0], -a[1])

    def cadd(a, c):
        return (a[0] + c[0], a[1] + c[1])

    def csub(a, c):
        return (a[0] - c[0], a[1] - c[1])

    bnrm = nrm(b)
    m1 = m + 1
    V = np.zeros((n, m1), dtype=T, order="F")
    Hr, Hi = np.zeros((m1, m), dtype=T), np.zeros((m1, m), dtype=T)
    cs, sn = [(T(0), T(0))] * m, [(T(0), T(0))] * m
    info = dict(success=False, num_matvec=0, res_norm=[], res_norm_unrounded=[], num_iter=0, cycles=[])

    r = b - np.asarray(apply(x), dtype=T)
    info["num_matvec"] += 1
    r_nrm = nrm(r)
    info["res_norm"].append(float(r_nrm))
    info["res_norm_unrounded"].append(r_nrm)
    if r_nrm < T(tol) * bnrm:
        info["success"] = True
        return x, info
    it = 1
    while it < maxit:
        V[:, 0] = (one / r_nrm) * r
        eta = [(T(0), T(0))] * m1
        eta[0] = (r_nrm, T(0))
        k1 = 0
        for j in range(m):
            k1 = j + 1
            w = np.asarray(apply(V[:, j]), dtype=T)
            info["num_matvec"] += 1
            wr, wi = w[:h].copy(), w[h:].copy()
            col = []
            for i in range(k1):
                vr, vi = V[:h, i], V[h:, i]
                c = (dot(wr, vr) + dot(wi, vi), dot(wi, vr) - dot(wr, vi))
                wr, wi = wr - (c[0] * vr - c[1] * vi), wi - (c[0] * vi + c[1] * vr)
                col.append(c)
            col.append((T(np.sqrt(dot(wr, wr) + dot(wi, wi))), T(0)))
            if col[k1][0] == 0:
                Hr[:k1 + 1, j], Hi[:k1 + 1, j] = [c[0] for c in col], [c[1] for c in col]
                break
            inv = one / col[k1][0]
            V[:h, k1], V[h:, k1] = wr * inv, wi * inv
            for i in range(j):
                h1, h2 = col[i], col[i + 1]
                col[i] = cadd(cmul(conj(cs[i]), h1), cmul(conj(sn[i]), h2))
                col[i + 1] = csub(cmul(cs[i], h2), cmul(sn[i], h1))
            t = T(np.hypot(T(np.hypot(col[j][0], col[j][1])), T(np.hypot(col[j + 1][0], col[j + 1][1]))))
            cs[j] = (col[j][0] / t, col[j][1] / t)
            sn[j] = (col[j + 1][0] / t, col[j + 1][1] / t)
            col[j] = cadd(cmul(conj(cs[j]), col[j]), cmul(conj(sn[j]), col[j + 1]))
            col[j + 1] = (T(0), T(0))
            Hr[:k1 + 1, j], Hi[:k1 + 1, j] = [c[0] for c in col], [c[1] for c in col]
            e = cmul(sn[j], eta[j])
            eta[k1] = (-e[0], -e[1])
            eta[j] = cmul(conj(cs[j]), eta[j])
            if T(np.hypot(eta[k1][0], eta[k1][1])) < T(tol) * bnrm:
                break
        y = list(eta[:k1])
        for i in range(k1 - 1, -1, -1):
            s = y[i]
            for j in range(i + 1, k1):
                s = csub(s, cmul((Hr[i, j], Hi[i, j]), y[j]))
            y[i] = cdiv(s, (Hr[i, i], Hi[i, i]))
        info["cycles"].append(k1)
        for j in range(k1):
            vr, vi = V[:h, j], V[h:, j]
            x = np.concatenate([x[:h] + (y[j][0] * vr - y[j][1] * vi), x[h:] + (y[j][0] * vi + y[j][1] * vr)])
        r = b - np.asarray(apply(x), dtype=T)
        info["num_matvec"] += 1
        r_nrm = nrm(r)
        info["res_norm"].append(float(r_nrm))
        info["res_norm_unrounded"].append(r_nrm)
        if r_nrm < T(tol) * bnrm:
            info["success"] = True
            break
        it += 1
    info["num_iter"] = it
    return x, info


# ---------------------------------------------------------------- the model in longdouble on the trace system, frozen
# tests/test_gpu_gmres_complex.py bounds the device's distance from the float64 model by the model's own sensitivity: float64
# against longdouble on the same matrix.  The longdouble run multiplies a 3,136 x 3,136 matrix 141 times without BLAS (8 s), so its
# residual norms are frozen in tests/golden/cgmres_trace_longdouble.npz as float64 pairs hi + lo, with the counts.
# tests/test_cgmres_reference.py recomputes the first cycles against the file.  Regenerate:  python tests/cgmres_reference.py
TRACE_RUN = dict(m=20, maxit=61, tol=1e-6)


def trace_longdouble(maxit=TRACE_RUN["maxit"]):
    """(res_hi, res_lo, num_matvec, cycles) of the longdouble model on lgmres_reference.trace_system(*TRACE_CASE)"""
    import lgmres_reference as lr

    A, b = lr.trace_system(*lr.TRACE_CASE)
    _, info = cgmres_ref(A, b, TRACE_RUN["m"], maxit, TRACE_RUN["tol"], np.longdouble)
    r = np.asarray(info["res_norm_unrounded"], dtype=np.longdouble)
    hi = r.astype(np.float64)
    return hi, (r - hi).astype(np.float64), info["num_matvec"], np.asarray(info["cycles"])


def golden_path():
    import pathlib

    return pathlib.Path(__file__).resolve().parent / "golden" / "cgmres_trace_longdouble.npz"


if __name__ == "__main__":
    import sys

    sys.path.insert(0, str(golden_path().parents[2]))
    hi, lo, nmv, cycles = trace_longdouble()
    np.savez(golden_path(), res_hi=hi, res_lo=lo, num_matvec=nmv, cycles=cycles)
    print(f"{golden_path()}: {len(hi)} residual norms, {nmv} matvecs, cycles {cycles.tolist()}")
