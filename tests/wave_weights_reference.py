"""The stiffness of  -div(beta grad .)  with beta constant on each element, restated in numpy on dense matrices (TEST
INFRASTRUCTURE for the weighted lattice sweeps).

    K_beta = sum_e beta_e P_e^T K_el P_e,      K_el = cx (A (x) diag w) + cy (diag w (x) A),   cx = hy / hx,  cy = hx / hy,

A = D^T diag(w) D and w the 1-D tables of the product (cuddh_wave_lattice_tables), P_e the element's node list from the space
(global_indices: node (i, j) of element e, i along x).  Local index i + n_basis j:
    K_el[(i, j), (i', j')] = cx A[i, i'] w[j] [j = j'] + cy w[i] [i = i'] A[j, j'].
`model` hands K_beta to waveholtz_reference.Model with lumped()'s m and h: mass and faces do not depend on beta.
"""
from __future__ import annotations

import math

import numpy as np

import waveholtz_reference as wr


def tables(nb):
    import cuddhelmholtz_amd as cd
    from cuddhelmholtz_amd import _native as N

    A, w, basis = np.zeros((nb, nb)), np.zeros(nb), cd.Basis(nb)
    N.check_capi(N.lib.cuddh_wave_lattice_tables(basis._h, A.ctypes.data, w.ctypes.data))
    return A, w


def element_matrix(A, w, cx, cy):
    """K_el on the local index i + n_basis j"""
    return cx * np.kron(np.diag(w), A) + cy * np.kron(A, np.diag(w))


def weighted_stiffness(fem, hx, hy, beta) -> np.ndarray:
    """dense K_beta on the dofs of the space `fem` (cd.H1Space over congruent hx x hy rectangles)"""
    nb = fem.basis.n
    A, w = tables(nb)
    K_el = element_matrix(A, w, hy / hx, hx / hy)
    I = fem.global_indices()  # (nb, nb, n_elem): I[i, j, e]
    beta = np.asarray(beta, dtype=np.float64)
    assert beta.shape == (I.shape[2],)
    K = np.zeros((fem.size(), fem.size()))
    for e in range(I.shape[2]):
        nodes = I[:, :, e].reshape(-1, order="F")  # i + nb j
        K[np.ix_(nodes, nodes)] += beta[e] * K_el
    return K


def beta_ratio(h_a, I, beta) -> int:
    """the time ratio a (a, beta) medium asks for: max(1, ceil((1 - 1e-9) max_e sqrt(beta_e) / min_{g in e} a_g)); I (.., n_elem)"""
    h_a, beta = np.asarray(h_a, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    nodes = np.asarray(I).reshape(-1, beta.size, order="F")
    speed = float(np.max(np.sqrt(beta) / h_a[nodes].min(axis=0)))
    return max(1, int(math.ceil(speed * (1.0 - 1e-9))))


def model(c: wr.Case, K_beta, scheme="rk2", coarsen=1, ratio=1, faces=None) -> wr.Model:
    """waveholtz_reference.Model on K_beta with lumped()'s m and h of the case's discretisation"""
    m, h = c.mh if faces is None else wr.lumped(c.d, faces)
    return wr.Model(K_beta, m, h, c.h_a, c.omega, c.nt(coarsen, ratio), scheme)
