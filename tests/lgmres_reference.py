"""Restarted GMRES augmented with the last k corrections (LGMRES, Baker, Jessup and Manteuffel) restated in numpy, and the
exact-local-solve trace system it was measured on (TEST INFRASTRUCTURE, not collected).

Shared by tests/test_lgmres_reference.py (CPU: pins `lgmres_ref` with k = 0 to cgs2_reference.gmres_cgs2_ref, which is pinned to
oracle.gmres, and checks what augmentation promises) and tests/test_gpu_gmres_augment.py (gmres(..., augment=k) on the device).

The iteration (krylov.cpp::arnoldi_restarted, augment = k): a cycle has at most m columns.  With ka = min(k, pairs stored),
columns j < m - ka are Krylov columns (u_j = v_j, w = A v_j, one operator application); column m - ka + p is an augmentation
column (u_j = z_p, w = the stored A z_p, no operator application).  w is orthogonalised against v_0..v_j and normalised into
v_{j+1}; Givens rotations, inner exit and breakdown rule as in oracle.gmres.  End of cycle: dx = sum_j y_j u_j (from 0, ascending
j), x <- x + dx, the true residual, and, when another cycle follows and |dx| > 0, the new pair z = dx / |dx|,
A z = (r_old - r_new) / |dx| in front of the others (at most k are kept).
"""
from __future__ import annotations

import math

import numpy as np

import cgs2_reference as cr


def lgmres_ref(A, b, m, maxit, tol, k, T=np.float64, x0=None, orth="mgs", record=False):
    """A: a matrix or a callable x -> A x.  Every operation in `T`.  Returns (x, info); info as gmres_cgs2_ref's, and
    "cycles": per cycle (columns, Krylov columns among them), "pairs": the (z, A z) stored at the end, most recent first;
    record=True adds "history": per cycle dict(r_old, r_new, U: the explicit columns u_j, pairs: those stored after the cycle)."""
    if not (isinstance(k, (int, np.integer)) and 0 <= k and (k == 0 or k < m)):
        raise ValueError(f"augment must be an integer in [0, m - 1], not {k!r}")
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
    info = dict(success=False, num_matvec=0, res_norm=[], res_norm_unrounded=[], num_iter=0, cycles=[], pairs=[], history=[])
    pairs = info["pairs"]

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
        n_krylov = m - min(k, len(pairs))
        U = []
        k1 = 0
        for j in range(m):
            k1 = j + 1
            if j < n_krylov:
                U.append(V[:, j].copy())
                w = np.asarray(apply(V[:, j]), dtype=T)
                info["num_matvec"] += 1
            else:
                z, Az = pairs[j - n_krylov]
                U.append(z)
                w = Az.copy()
            basis = [V[:, i] for i in range(k1)]
            if orth == "cgs2":
                _, w, dA, _ = cr.cgs_pass_ref(w, basis, precision=T)
                c1, w, dB, _ = cr.cgs_pass_ref(w, basis, c=dA, precision=T)
                hk, w, _, ww = cr.cgs_pass_ref(w, basis, c=dB, hacc=c1, dots=False, precision=T)
                H[:k1, j] = hk
                H[k1, j] = T(np.sqrt(T(ww)))
            elif orth == "mgs":
                hk, w = cr.mgs_step_ref(w, basis, T)
                H[:k1 + 1, j] = hk
            else:
                raise ValueError(orth)
            if H[k1, j] == 0:
                break
            V[:, k1] = w * (one / H[k1, j])
            h = H[:, j]
            for i in range(j):
                h1, h2 = h[i], h[i + 1]
                h[i] = cs[i] * h1 + sn[i] * h2
                h[i + 1] = -sn[i] * h1 + cs[i] * h2
            t = T(np.hypot(h[j], h[j + 1]))
            cs[j] = h[j] / t
            sn[j] = h[j + 1] / t
            h[j] = cs[j] * h[j] + sn[j] * h[j + 1]
            h[j + 1] = 0
            eta[k1] = -sn[j] * eta[j]
            eta[j] = cs[j] * eta[j]
            if abs(eta[k1]) < T(tol) * bnrm:
                break
        yk = eta[:k1].copy()
        for i in range(k1 - 1, -1, -1):
            s = yk[i]
            for j in range(i + 1, k1):
                s -= H[i, j] * yk[j]
            yk[i] = s / H[i, i]
        info["cycles"].append((k1, min(k1, n_krylov)))
        dx_nrm = T(0)
        if k == 0:
            for j in range(k1):
                x = x + yk[j] * V[:, j]
        else:
            dx = np.zeros(n, dtype=T)
            for j in range(k1):
                dx = dx + yk[j] * U[j]
            x = x + dx
            dx_nrm = nrm(dx)
        r_old = r
        r = b - np.asarray(apply(x), dtype=T)
        info["num_matvec"] += 1
        r_nrm = nrm(r)
        info["res_norm"].append(float(r_nrm))
        info["res_norm_unrounded"].append(r_nrm)
        done = r_nrm < T(tol) * bnrm
        if dx_nrm > 0 and not done:
            inv = one / dx_nrm
            pairs.insert(0, (inv * dx, (-inv) * r + inv * r_old))
            del pairs[k:]
        if record:
            info["history"].append(dict(r_old=r_old, r_new=r, U=np.stack(U[:k1], axis=1), pairs=list(pairs)))
        if done:
            info["success"] = True
            break
        it += 1
    info["num_iter"] = it
    return x, info


def block_labels(nx, ny, epd):
    ndx = nx // epd
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    return ((i // epd) + ndx * (j // epd)).reshape(-1).astype(np.int32)


def trace_system(nx, block, omega):
    """The trace system of DDH with EXACT local solves on uniform_rect(nx, -1, 1, nx, -1, 1), n_basis 4, a = 1, subdomains of
    block x block elements: (I - M, c) with M and c as ddh_general.fixed_point assembles them (it solves this system and returns
    only the postprocessed solution), complex n_lambda x n_lambda, returned as the real 2 n_lambda system [[Re, -Im], [Im, Re]]
    and [Re c; Im c].  Right-hand side: the Gaussian sources of the examples at this omega."""
    import ddh_general as dg
    import oracle

    nb = 4
    d = oracle.Discretization(oracle.Mesh.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), nb)
    h_a = np.ones(d.ndof)
    labels = block_labels(nx, nx, block)
    O = dg.OracleDDH(d, (nx // block) ** 2, labels, omega, h_a, np.float64)
    t, G, ndof = O.t, O.G, d.ndof
    load = oracle.linear_functional(d, oracle.gaussians(omega)).astype(np.complex128)

    # ddh_general.fixed_point, up to its solve
    nodes, nl, w = nb * nb, t.n_lambda, t.omega
    D = np.asarray(t.D, dtype=np.float64)
    M = np.zeros((nl, nl), dtype=np.complex128)
    c = np.zeros(nl, dtype=np.complex128)
    for s in range(t.n_domains):
        n, nf = int(t.s_dof[s]), int(t.s_fdof[s])
        S = np.zeros((n, n))
        for el in range(int(t.s_elems[s])):
            idx = t.sI[:, :, el, s].reshape(-1, order="F")
            S[np.ix_(idx, idx)] += dg.element_stiffness(D, G[:, el * nodes:(el + 1) * nodes, s])
        a = t.a[:n, s].astype(np.float64)
        Hs = np.zeros(n)
        Hs[:nf] = t.H[:nf, s]
        Ainv = np.linalg.inv(S.astype(np.complex128) + np.diag(-w * w * a * a * t.m[:n, s] + 1j * w * a * Hs))
        rd, wr = t.B[:nf, 0, s], t.B[:nf, 1, s]
        fr = np.flatnonzero(rd >= 0)
        R = np.zeros((n, nl), dtype=np.complex128)
        R[fr, rd[fr]] = Hs[fr]
        Uf, UL = Ainv @ load[t.gI[:n, s]], Ainv @ R
        for i in np.flatnonzero(wr >= 0):
            M[wr[i], :] = 2j * w * a[i] * UL[i, :]
            if rd[i] >= 0:
                M[wr[i], rd[i]] -= 1.0
            c[wr[i]] = 2j * w * a[i] * Uf[i]
    K = np.eye(nl) - M
    return np.block([[K.real, -K.imag], [K.imag, K.real]]), np.concatenate([c.real, c.imag])


TRACE_CASE = (16, 2, math.pi)  # elements per side, elements per subdomain side, omega: 3,136 real unknowns
