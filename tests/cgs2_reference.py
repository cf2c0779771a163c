"""CGS2 orthogonalisation (classical Gram-Schmidt applied twice) restated in numpy (TEST INFRASTRUCTURE, not collected).

Shared by tests/test_cgs2_reference.py (CPU: pins this module to oracle.gmres and to the orthogonality figures),
tests/test_gpu_cgs2_kernels.py (holds cgs_pass / cgs_reduce of kernels/blas1.hip to it) and tests/test_gpu_gmres_cgs2.py
(gmres(..., orth="cgs2")).  oracle.gmres is modified Gram-Schmidt only, so the reference of the option is `gmres_cgs2_ref`:
oracle.gmres's iteration, statement for statement, with the orthogonalisation of the Arnoldi step exchangeable.

A pass (blas1.hip::cgs_pass_kernel), against ALL basis vectors at once:
    update   h_out = (h_acc or 0) + c;   w <- w - sum_j c[j] v_j   (ascending j)
    dots     d[j] = <w, v_j> of the updated w, and <w, w>
A step:  pass A (dots), pass B (update with d_A, dots), pass C (update with d_B, h = d_A + d_B, <w, w>), normalisation.
"""
from __future__ import annotations

import numpy as np

import blas1_reference as br

KC = 4  # basis vectors per register chunk of cgs_pass_kernel (CGS_KC)
KMAX = 512  # largest k1 of one launch (CGS_KMAX)
ROW = br.MAX_PARTIALS  # scalars per row of a partial-sum buffer: row 0 <w, w>, row 1 + j <w, v_j>


def cgs_pass_ref(w, V, c=None, hacc=None, dots=True, precision=None, dtype="f64"):
    """One pass in `precision` (default: br.wide(dtype)).  Returns (hout or None, new w, d or None, <w, w>)."""
    W = br.wide(dtype) if precision is None else precision
    w = np.asarray(w).astype(W)
    Vw = [np.asarray(v).astype(W) for v in V]
    hout = None
    if c is not None:
        c = np.asarray(c).astype(W)
        hout = c.copy() if hacc is None else np.asarray(hacc).astype(W) + c
        for j, v in enumerate(Vw):
            w = w - c[j] * v
    d = np.asarray([np.dot(w, v) for v in Vw], dtype=W) if dots else None
    return hout, w, d, np.dot(w, w)


def cgs_step_ref(w, V, precision=None, dtype="f64"):
    """The CGS2 step on w against V: (h[0..k1], normalised w, c1) with h[k1] the norm, in `precision` (default br.wide(dtype))."""
    _, w, dA, _ = cgs_pass_ref(w, V, precision=precision, dtype=dtype)
    c1, w, dB, _ = cgs_pass_ref(w, V, c=dA, precision=precision, dtype=dtype)
    h, w, _, ww = cgs_pass_ref(w, V, c=dB, hacc=c1, dots=False, precision=precision, dtype=dtype)
    nrm = np.sqrt(ww)
    return np.append(h, nrm), w / nrm, c1


def mgs_step_ref(w, V, precision):
    """the Arnoldi step of oracle.gmres: (h[0..k1], w NOT normalised)"""
    h = []
    for v in V:
        hj = precision(np.dot(w, v))
        w = w - hj * v
        h.append(hj)
    h.append(precision(np.sqrt(precision(np.dot(w, w)))))
    return np.asarray(h, dtype=precision), w


def arnoldi_basis(diag, b, steps, dtype, orth):
    """`steps` Arnoldi steps on the diagonal operator `diag` from b, every operation in NP[dtype]: the basis as a list of vectors.
    orth "cgs2": cgs_step_ref in the working precision; "mgs": br.mgs_chain_ref (the chain krylov.cpp queues by default)."""
    T = br.NP[dtype]
    d = np.asarray(diag, dtype=T)
    v0 = np.asarray(b, dtype=T)
    V = [v0 / T(np.sqrt(np.dot(v0, v0)))]
    for _ in range(steps):
        w = d * V[-1]
        if orth == "cgs2":
            _, q, _ = cgs_step_ref(w, V, precision=T, dtype=dtype)
        else:
            _, q = br.mgs_chain_ref(w, V)
        V.append(np.asarray(q, dtype=T))
    return V


def orthogonality_loss(V, dtype) -> float:
    """max |V^T V - I| evaluated in the wide type"""
    Q = np.stack([np.asarray(v).astype(br.wide(dtype)) for v in V], axis=1)
    return float(np.max(np.abs(Q.T @ Q - np.eye(Q.shape[1], dtype=Q.dtype))))


def separation_case():
    """the input of the orthogonality tests: diagonal operator of condition 1e6 on 300 dofs, a fixed right-hand side, 20 steps"""
    return np.geomspace(1.0, 1e6, 300), np.random.default_rng(1).standard_normal(300), 20


def gmres_cgs2_ref(A, b, m=20, maxit=100, tol=1e-6, dtype=np.float64, orth="cgs2", x0=None):
    """oracle.gmres (source/gmres.cpp:91-235: cycle count, exit tests, breakdown rule, num_matvec, res_norm) with the Arnoldi step's
    orthogonalisation chosen: "cgs2", or "mgs" (then it is oracle.gmres itself: tests/test_cgs2_reference.py).  A: a matrix or a
    callable x -> A x.  Every operation in `dtype` (np.float32, np.float64 or np.longdouble).  Returns (x, info)."""
    T = dtype
    apply = (lambda v: A @ v) if isinstance(A, np.ndarray) else A
    if isinstance(A, np.ndarray):
        A = A.astype(T)
    n = len(b)
    b = np.asarray(b, dtype=T)
    x = np.zeros(n, dtype=T) if x0 is None else np.array(x0, dtype=T)
    one = T(1)

    def nrm(v):
        return T(np.sqrt(T(np.dot(v, v))))

    bnrm = nrm(b)
    m1 = m + 1
    V = np.zeros((n, m1), dtype=T, order="F")
    H = np.zeros((m1, m), dtype=T, order="F")
    sn, cs, eta = np.zeros(m, dtype=T), np.zeros(m, dtype=T), np.zeros(m1, dtype=T)
    info = dict(success=False, num_matvec=0, res_norm=[], res_norm_unrounded=[], num_iter=0)  # (unrounded: in `dtype`, not as float)

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
        eta[:] = 0
        eta[0] = r_nrm
        k1 = 0
        for k in range(m):
            k1 = k + 1
            w = np.asarray(apply(V[:, k]), dtype=T)
            info["num_matvec"] += 1
            basis = [V[:, j] for j in range(k1)]
            if orth == "cgs2":
                _, w, dA, _ = cgs_pass_ref(w, basis, precision=T)
                c1, w, dB, _ = cgs_pass_ref(w, basis, c=dA, precision=T)
                hk, w, _, ww = cgs_pass_ref(w, basis, c=dB, hacc=c1, dots=False, precision=T)
                H[:k1, k] = hk
                H[k1, k] = T(np.sqrt(T(ww)))
            elif orth == "mgs":
                hk, w = mgs_step_ref(w, basis, T)
                H[:k1 + 1, k] = hk
            else:
                raise ValueError(orth)
            if H[k1, k] == 0:
                break
            V[:, k1] = w * (one / H[k1, k])
            h = H[:, k]
            for i in range(k):
                h1, h2 = h[i], h[i + 1]
                h[i] = cs[i] * h1 + sn[i] * h2
                h[i + 1] = -sn[i] * h1 + cs[i] * h2
            t = T(np.hypot(h[k], h[k + 1]))
            cs[k] = h[k] / t
            sn[k] = h[k + 1] / t
            h[k] = cs[k] * h[k] + sn[k] * h[k + 1]
            h[k + 1] = 0
            eta[k1] = -sn[k] * eta[k]
            eta[k] = cs[k] * eta[k]
            if abs(eta[k1]) < T(tol) * bnrm:
                break
        yk = eta[:k1].copy()
        for i in range(k1 - 1, -1, -1):
            s = yk[i]
            for j in range(i + 1, k1):
                s -= H[i, j] * yk[j]
            yk[i] = s / H[i, i]
        for k in range(k1):
            x = x + yk[k] * V[:, k]
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


# ---------------------------------------------------------------- exact-integer case of the kernel tests
def exact_cgs(n: int, dtype: str, k1: int, rng):
    """w in {-2..2} and k1 sparse +-1 basis vectors: br.sparse_signs with the distinct shifts 0..k1-1 (a handful of nonzeros at
    the first element, the tile boundaries, the last full 16-byte vector and the tail, moved by the shift), each without the places
    an earlier one holds.  The supports are disjoint, so a coefficient grows by at most the factor (nonzeros - 1) <= 5 per pass and
    every sum stays far below br.EXACT_LIMIT (`exact_step` returns the largest; the caller checks it): every summation order
    gives the same bits.  Vectors whose places are all taken are zero (tiny n)."""
    wmax = 2 if 4 * n + 4096 <= br.EXACT_LIMIT[dtype] else 1  # ({-1..1} where 4 n would pass the exactness limit, as br.exact_mgs)
    w = rng.integers(-wmax, wmax + 1, n, dtype=np.int8).astype(np.int64)
    V, taken = [], np.zeros(n, dtype=bool)
    for j in range(k1):
        v = br.sparse_signs(n, dtype, shift=j).astype(np.int64)
        v[taken] = 0
        taken |= v != 0
        V.append(v)
    for v in V:
        w[v != 0] = wmax * v[v != 0]  # every term of <w, v_j> is + wmax: no coefficient of a nonzero vector is zero
    return w, V


def exact_step(w, V):
    """the three passes in Python integers (int64): dict of everything a pass leaves behind"""
    w = np.asarray(w, dtype=np.int64)
    dA = np.array([int(np.dot(w, v)) for v in V], dtype=np.int64)
    wwA = int(np.dot(w, w))
    wB = w - sum(int(c) * v for c, v in zip(dA, V))
    dB = np.array([int(np.dot(wB, v)) for v in V], dtype=np.int64)
    wwB = int(np.dot(wB, wB))
    wC = wB - sum(int(c) * v for c, v in zip(dB, V))
    wwC = int(np.dot(wC, wC))
    largest = max([wwA, wwB, wwC] + [int(np.sum(np.abs(x * v))) for x in (w, wB) for v in V] + [int(np.max(np.abs(dA + dB), initial=0))])
    return dict(dA=dA, wwA=wwA, wB=wB, dB=dB, wwB=wwB, wC=wC, wwC=wwC, h=dA + dB, largest=largest)
