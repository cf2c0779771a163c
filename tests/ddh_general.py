"""DDH on subdomains given by element labels, restated on the test side (TEST INFRASTRUCTURE).

oracle.numbering.ddh_tables is fixed to blocks of uniform_rect meshes.  `tables` below takes any labels: it calls
oracle.numbering.ensemble(...) and restates only the part of ddh_tables that does not depend on how the labels were made
(time grid, slot table B, face-first renumbering, lumped masses, H, a).  `tables` is proven against ddh_tables on block
labels (tests/test_ddh_labels.py) before anything relies on it.

`OracleDDH` runs the oracle's table-driven local solves (orc_ddh_apply_*) on such tables.  `fixed_point` is what DDH with
EXACT local solves converges to, for any labels: every subdomain s solves
    (S_s - w^2 a^2 m_s + i w a H_s) U_s = f|_s + H_s L_read(s)
and writes -L + 2 i w a U_s into its write slots (slots from B); the result is the partition-of-unity average of
DDH::postprocess.  It is proven against helmholtz_direct.ddh_fixed_point_solution on block decompositions.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

import oracle
from oracle.numbering import DdhTables, ensemble


def tables(mesh, I, ndof, n_domains, labels, omega, h_a, gll_x, gll_w, Dmat, detJ, real=np.float32) -> DdhTables:
    """ddh_tables for arbitrary element labels; nel1d is 0."""
    nb = I.shape[0]
    ens = ensemble(mesh, I, n_domains, labels)

    T = 2 * math.pi / omega
    h = mesh.min_h()
    dt = 0.2 * 0.5 * h / (nb * nb)
    nt = int(math.ceil(T / dt))
    dt = T / nt
    filt = np.zeros(nt + 1, dtype=real)
    for k in range(nt + 1):
        filt[k] = dt * (omega / math.pi) * (math.cos(omega * k * dt) - 0.25)
    filt[0] = real(filt[0] * 0.5)
    filt[nt] = real(filt[nt] * 0.5)
    cs = np.zeros(2 * nt + 1, dtype=real)
    sn = np.zeros(2 * nt + 1, dtype=real)
    for k in range(2 * nt + 1):
        t = 0.5 * k * dt
        cs[k] = -math.cos(omega * t)
        sn[k] = math.sin(omega * t)

    mx_dof, mx_fdof, mx_el = int(ens.s_dof.max()), int(ens.s_fdof.max()), int(ens.s_elems.max())
    n_shared = ens.cmap.shape[1]
    n_lambda = 2 * n_shared
    B = -np.ones((mx_fdof, 2, n_domains), dtype=np.int32, order="F")
    for k in range(n_shared):
        S0, S1, j0, j1 = (int(v) for v in ens.cmap[:, k])
        B[j0, 0, S0] = k
        B[j0, 1, S0] = n_shared + k
        B[j1, 0, S1] = n_shared + k
        B[j1, 1, S1] = k
    used = set(int(v) for v in B.reshape(-1) if v >= 0)
    orphan = 2 * (n_lambda - len(used))

    gI = -np.ones((mx_dof, n_domains), dtype=np.int32, order="F")
    sI = -np.ones((nb, nb, mx_el, n_domains), dtype=np.int32, order="F")
    for s in range(n_domains):
        nd, nf = int(ens.s_dof[s]), int(ens.s_fdof[s])
        face = [int(ens.pI[l, s]) for l in range(nf)]
        fs = set(face)
        perm = np.asarray(face + [i for i in range(nd) if i not in fs], dtype=np.int64)
        inv = np.empty(nd, dtype=np.int64)
        inv[perm] = np.arange(nd)
        gI[:nd, s] = ens.gI[perm, s]
        ne = int(ens.s_elems[s])
        sI[:, :, :ne, s] = inv[ens.sI[:, :, :ne, s]]

    mi = np.zeros(ndof)
    for el in range(mesh.n_elem):
        for j in range(nb):
            for i in range(nb):
                mi[I[i, j, el]] += gll_w[i] * gll_w[j] * detJ[i, j, el]
    mi = 1.0 / mi

    m = np.zeros((mx_dof, n_domains), dtype=real, order="F")
    H = np.zeros((mx_fdof, n_domains), dtype=real, order="F")
    A = np.zeros((mx_dof, n_domains), dtype=real, order="F")
    gmi = np.zeros((mx_dof, n_domains), dtype=real, order="F")
    for s in range(n_domains):
        for el in range(ens.s_elems[s]):
            g_el = ens.elems[el, s]
            for j in range(nb):
                for i in range(nb):
                    l = sI[i, j, el, s]
                    m[l, s] = real(float(m[l, s]) + gll_w[i] * gll_w[j] * detJ[i, j, g_el])
        nd = int(ens.s_dof[s])
        A[:nd, s] = h_a[gI[:nd, s]]
        gmi[:nd, s] = mi[gI[:nd, s]]
        for f in range(ens.s_faces[s]):
            e = mesh.edges[ens.faces[f, s]]
            for i in range(nb):
                l = ens.fI[i, f, s]
                H[l, s] = real(float(H[l, s]) + (e.length / 2) * gll_w[i])

    return DdhTables(n_domains, n_lambda, nt, dt, float(omega), nb, 0, mx_dof, mx_fdof, mx_el, ens.s_dof, ens.s_fdof, ens.s_elems, ens.elems,
                     B, gI, sI, np.asarray(Dmat, dtype=real, order="F"), m, gmi, A, H, filt, cs, sn, ens, orphan)


class OracleDDH(oracle.DDH):
    """oracle.DDH on tables from `tables` (any labels)."""

    def __init__(self, disc, n_domains, labels, omega, h_a, real=np.float32):
        self.d, self.real = disc, real
        nb = disc.nb
        _, Dm = oracle.basis_tables(nb, disc.gll_x)
        J, detJ, _ = disc.metrics(disc.gll_x)
        self.t = tables(disc.mesh, disc.I, disc.ndof, n_domains, labels, omega, np.asarray(h_a, dtype=np.float64), disc.gll_x, disc.gll_w, Dm,
                        detJ, real)
        t = self.t
        self.G = np.zeros((3, nb * nb * t.mx_elems, t.n_domains), dtype=real, order="F")
        fn = oracle.lib().orc_ddh_geom_f32 if real == np.float32 else oracle.lib().orc_ddh_geom_f64
        fn(C.c_int(t.n_domains), C.c_int(t.mx_elems), C.c_int(nb), oracle._p(np.ascontiguousarray(t.s_elems, dtype=np.int32)),
           oracle._p(np.asfortranarray(t.elems, dtype=np.int32)), oracle._p(disc.gll_w), oracle._p(J), oracle._p(self.G))
        self.size = 2 * t.n_lambda
        # The oracle's sweep indexes its LDS restatement with sI also for element nodes past a subdomain's elements (their G is
        # zero, so they add exact zeros); point those at dof 0 instead of -1 so that nothing outside its buffers is touched.
        self._sI_product = t.sI
        t.sI = np.where(t.sI < 0, 0, t.sI).astype(np.int32, order="F")


def element_stiffness(D, g):
    """S_el (nb^2 x nb^2, node k + nb l) of one element from its factors g (3, nb^2): the sweep of source/DDH.cpp:60-109 as a matrix"""
    nb = D.shape[0]
    Dx = np.kron(np.eye(nb), D)  # ux(k, l) = sum_i D(k, i) u(i, l)
    Dy = np.kron(D, np.eye(nb))  # uy(k, l) = sum_i D(l, i) u(k, i)
    return (Dx.T @ (g[0][:, None] * Dx) + Dx.T @ (g[1][:, None] * Dy) + Dy.T @ (g[1][:, None] * Dx) + Dy.T @ (g[2][:, None] * Dy))


def fixed_point(t: DdhTables, G, ndof: int, f: np.ndarray):
    """The solution DDH with exact local solves converges to (module docstring), as the 2*ndof real vector of postprocess.
    t: fp64 tables, G: fp64 geometric factors (3, nb*nb*mx_elems, n_domains), f: the 2*ndof load."""
    nb, nd, nl = t.nb, t.n_domains, t.n_lambda
    D = np.asarray(t.D, dtype=np.float64)
    w = t.omega
    load = f[:ndof] + 1j * f[ndof:]
    nodes = nb * nb
    local = []
    # per subdomain: U = Ainv (f_s + H_s L_read);  written traces  L'[w] = -L[r] + 2 i w a U
    M = np.zeros((nl, nl), dtype=np.complex128)
    c = np.zeros(nl, dtype=np.complex128)
    for s in range(nd):
        n, nf = int(t.s_dof[s]), int(t.s_fdof[s])
        S = np.zeros((n, n))
        for el in range(int(t.s_elems[s])):
            idx = t.sI[:, :, el, s].reshape(-1, order="F")
            Ke = element_stiffness(D, G[:, el * nodes:(el + 1) * nodes, s])
            S[np.ix_(idx, idx)] += Ke
        a = t.a[:n, s].astype(np.float64)
        H = np.zeros(n)
        H[:nf] = t.H[:nf, s]
        A = S.astype(np.complex128) + np.diag(-w * w * a * a * t.m[:n, s] + 1j * w * a * H)
        Ainv = np.linalg.inv(A)
        rd, wr = t.B[:nf, 0, s], t.B[:nf, 1, s]
        fr = np.flatnonzero(rd >= 0)
        R = np.zeros((n, nl), dtype=np.complex128)  # f_s + H_s L_read = fs + R L
        R[fr, rd[fr]] = H[fr]
        fs = load[t.gI[:n, s]]
        Uf, UL = Ainv @ fs, Ainv @ R
        for i in np.flatnonzero(wr >= 0):
            M[wr[i], :] = 2j * w * a[i] * UL[i, :]
            if rd[i] >= 0:
                M[wr[i], rd[i]] -= 1.0
            c[wr[i]] = 2j * w * a[i] * Uf[i]
        local.append((n, Uf, UL))
    L = np.linalg.solve(np.eye(nl) - M, c)
    y = np.zeros(ndof, dtype=np.complex128)
    for s, (n, Uf, UL) in enumerate(local):
        U = Uf + UL @ L
        np.add.at(y, t.gI[:n, s], t.m[:n, s] * t.gmi[:n, s] * U)
    return np.concatenate([y.real, y.imag])


def morton_labels(centroids: np.ndarray, per_part: int = 16) -> np.ndarray:
    """Elements in Morton (Z) order of their centroids, cut into consecutive runs of per_part elements."""
    lo, hi = centroids.min(0), centroids.max(0)
    q = np.clip(((centroids - lo) / (hi - lo + 1e-300) * 65535).astype(np.int64), 0, 65535)

    def spread(v):
        v = (v | (v << 8)) & 0x00FF00FF
        v = (v | (v << 4)) & 0x0F0F0F0F
        v = (v | (v << 2)) & 0x33333333
        return (v | (v << 1)) & 0x55555555

    code = spread(q[:, 0]) | (spread(q[:, 1]) << 1)
    order = np.argsort(code, kind="stable")
    labels = np.empty(len(centroids), dtype=np.int32)
    labels[order] = np.arange(len(centroids)) // per_part
    return labels


def with_whole_star(labels: np.ndarray, elems: np.ndarray, vertex: int) -> np.ndarray:
    """labels with every element around `vertex` moved into one subdomain of its own; labels renumbered compactly"""
    star = np.flatnonzero((elems == vertex).any(axis=1))
    out = labels.astype(np.int64).copy()
    out[star] = out.max() + 1
    _, out = np.unique(out, return_inverse=True)
    return out.astype(np.int32)


def whole_stars(labels: np.ndarray, elems: np.ndarray, min_valence: int = 5):
    """vertices of valence >= min_valence whose whole element star lies in one subdomain"""
    val = np.bincount(elems.ravel())
    out = []
    for v in np.flatnonzero(val >= min_valence):
        star = np.flatnonzero((elems == v).any(axis=1))
        if np.unique(labels[star]).size == 1:
            out.append(int(v))
    return out
