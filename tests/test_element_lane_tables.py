"""The table of the element-lane DDH kernels (5, 11: n_basis 4; 12: n_basis 5), csrc/src/element_lane_tables.cpp, through
cuddh_element_lane_tables.  Host code: no GPU.

For the metric of a square element and of a 3:2 rectangle (the oracle's float factors, orc_ddh_geom_f32, of a one-element mesh):
    W (.) (Dg w + sum_{j != k} Bx(k,j) w(j,l) + sum_{j != l} By(l,j) w(k,j))  ==  ddh_general.element_stiffness(D, g) @ w
for random w, evaluated in double from the float table.  Tolerance, per node, all measured here and none taken from the result:
  * the table's float rounding: the difference of the float table to the same table formed in double here (table64, with the
    true weight gamma_k beta_l of every node), propagated through the expression with absolute values;
  * what the float metric itself lacks of being a product of 1-D factors (g is rounded to float node by node, the table
    is built from its first row and column): |S - S_separable| |w| with the residuals as they are;
  * 1e-13 of the row's scale for the double arithmetic of the test.
A metric with gy != 0 and one whose weight differs across a shared edge, W(nb-1, l) != W(0, l), are refused with -1, another
n_basis with 1 (hipErrorInvalidValue)."""
import ctypes as C

import numpy as np
import pytest

import ddh_general as dg
import oracle
from cuddhelmholtz_amd._native import lib


def element(nb, hx, hy):
    """D (nb, nb) and g (3, nb^2) in float, of one hx x hy element"""
    d = oracle.Discretization(oracle.Mesh.uniform_rect(1, 0.0, hx, 1, 0.0, hy), nb)
    _, Dm = oracle.basis_tables(nb, d.gll_x)
    J, _, _ = d.metrics(d.gll_x)
    G = np.zeros((3, nb * nb, 1), dtype=np.float32, order="F")
    oracle.lib().orc_ddh_geom_f32(C.c_int(1), C.c_int(1), C.c_int(nb), oracle._p(np.ones(1, dtype=np.int32)),
                                  oracle._p(np.zeros((1, 1), dtype=np.int32, order="F")), oracle._p(d.gll_w), oracle._p(J), oracle._p(G))
    return np.asarray(Dm, dtype=np.float32), G[:, :, 0].copy()


def tables(nb, D, g):
    """(error, table or None) of the export; D[a, b] = D(a, b), g[c, k + nb l]"""
    hD = np.asfortranarray(D, dtype=np.float32)
    hG = np.asfortranarray(g, dtype=np.float32)
    out = np.full(5 * nb * nb, np.nan, dtype=np.float32)
    err = lib.cuddh_element_lane_tables(nb, hD.ctypes.data, hG.ctypes.data, out.ctypes.data)
    if err:
        assert np.isnan(out).all()  # not written
        return err, None
    return 0, out


def table64(nb, D, g):
    """the table's definition in double: Bx, By, Dg, W (nb, nb) with [a, b] as the table indexes them, and the 1-D factors"""
    D = D.astype(np.float64)
    gx, gz = g[0].astype(np.float64).reshape(nb, nb, order="F"), g[2].astype(np.float64).reshape(nb, nb, order="F")  # [k, l]
    alpha, beta = gx[:, 0], gx[0, :] / gx[0, 0]
    gamma, delta = gz[:, 0] / gz[0, 0], gz[0, :]
    Ax, Ay = D.T @ (alpha[:, None] * D), D.T @ (delta[:, None] * D)
    Bx, By = Ax / gamma[:, None], Ay / beta[:, None]
    Dg = np.diag(Bx)[:, None] + np.diag(By)[None, :]
    return Bx, By, Dg, np.outer(gamma, beta), (alpha, beta, gamma, delta)


def sweep(nb, Bx, By, Dg, W, w):
    """W (.) z' with z' as the kernels form it; w, result [k, l]"""
    z = Dg * w
    for k in range(nb):
        for l in range(nb):
            z[k, l] += sum(Bx[k, j] * w[j, l] for j in range(nb) if j != k) + sum(By[l, j] * w[k, j] for j in range(nb) if j != l)
    return W * z, z


@pytest.mark.parametrize("hx,hy", [(1.0, 1.0), (3.0, 2.0)], ids=["square", "3:2"])
@pytest.mark.parametrize("nb", [4, 5])
def test_table_reproduces_the_element_stiffness_matrix(nb, hx, hy):
    D, g = element(nb, hx, hy)
    err, T = tables(nb, D, g)
    assert err == 0
    nn = nb * nb
    part = lambda i: T[i * nn:(i + 1) * nn].astype(np.float64).reshape(nb, nb, order="F")  # noqa: E731
    Bx, By, Dg, W, rW = (part(i) for i in range(5))
    Bx64, By64, Dg64, W64, (alpha, beta, gamma, delta) = table64(nb, D, g)
    dBx, dBy, dDg, dW = abs(Bx - Bx64), abs(By - By64), abs(Dg - Dg64), abs(W - W64)
    # float rounding of every entry (2^-24 relative) and, for W on the last nodes, the weight of the copy it is assembled with
    assert (dBx <= 2.0 ** -23 * abs(Bx64)).all() and (dBy <= 2.0 ** -23 * abs(By64)).all() and (dDg <= 2.0 ** -23 * abs(Dg64)).all()
    assert (dW <= 1e-6 * W64.max()).all() and (dW[:-1, :-1] <= 2.0 ** -23 * W64[:-1, :-1]).all()
    assert (W[-1, :] == W[0, :]).all() and (W[:, -1] == W[:, 0]).all()
    assert (abs(rW * W - 1.0) <= 2.0 ** -22).all()

    S = dg.element_stiffness(D.astype(np.float64), g.astype(np.float64))
    # the separable matrix the table stands for, and the entrywise distance of S to it
    Dd = D.astype(np.float64)
    Dx, Dy = np.kron(np.eye(nb), Dd), np.kron(Dd, np.eye(nb))
    rx = abs(g[0].astype(np.float64) - np.outer(alpha, beta).reshape(-1, order="F"))
    rz = abs(g[2].astype(np.float64) - np.outer(gamma, delta).reshape(-1, order="F"))
    assert (g[1] == 0).all()
    dS = abs(Dx).T @ (rx[:, None] * abs(Dx)) + abs(Dy).T @ (rz[:, None] * abs(Dy))

    rng = np.random.default_rng(nb)
    for _ in range(4):
        w = rng.standard_normal((nb, nb))
        got, _ = sweep(nb, Bx, By, Dg, W, w)
        _, z64 = sweep(nb, Bx64, By64, Dg64, W64, w)
        want = (S @ w.reshape(-1, order="F")).reshape(nb, nb, order="F")
        rounding, _ = sweep(nb, dBx, dBy, dDg, W, abs(w))
        scale = (abs(S) @ abs(w).reshape(-1, order="F")).reshape(nb, nb, order="F")
        tol = rounding + dW * abs(z64) + (dS @ abs(w).reshape(-1, order="F")).reshape(nb, nb, order="F") + 1e-13 * scale
        e = abs(got - want)
        print(f"[n_basis {nb}, {hx:g} x {hy:g}] max error {e.max():.3e}, tolerance there {tol.reshape(-1)[e.argmax()]:.3e}, row scale "
              f"{scale.reshape(-1)[e.argmax()]:.3e}")
        assert (e <= tol).all(), (e / tol).max()
        assert (tol <= 1e-5 * scale.max()).all()  # the tolerance is float rounding, not a licence


@pytest.mark.parametrize("nb", [4, 5])
def test_refusals(nb):
    D, g = element(nb, 3.0, 2.0)
    assert tables(nb, D, g)[0] == 0
    shear = g.copy()
    shear[1] = 0.1 * g[0]
    assert tables(nb, D, shear)[0] == -1
    # still a product of 1-D factors, but gamma_{nb-1} != gamma_0: the two copies of a node on a shared edge would scale differently
    uneven = g.copy().reshape(3, nb, nb, order="F")
    uneven[2, nb - 1, :] *= np.float32(1.01)
    assert tables(nb, D, uneven.reshape(3, nb * nb, order="F"))[0] == -1
    uneven = g.copy().reshape(3, nb, nb, order="F")
    uneven[0, :, nb - 1] *= np.float32(1.01)  # beta_{nb-1} != beta_0
    assert tables(nb, D, uneven.reshape(3, nb * nb, order="F"))[0] == -1
    bent = g.copy()
    bent[0, 1 + nb] *= np.float32(1.001)  # one node off the product form
    assert tables(nb, D, bent)[0] == -1


def test_other_orders_and_null_pointers_are_invalid_values():
    D, g = element(4, 1.0, 1.0)
    out = np.zeros(5 * 36, dtype=np.float32)
    hD, hG = np.asfortranarray(D), np.asfortranarray(g)
    for nb in (3, 6, 8, 0):
        assert lib.cuddh_element_lane_tables(nb, hD.ctypes.data, hG.ctypes.data, out.ctypes.data) == 1
    assert lib.cuddh_element_lane_tables(4, None, hG.ctypes.data, out.ctypes.data) == 1
    assert lib.cuddh_element_lane_tables(4, hD.ctypes.data, None, out.ctypes.data) == 1
    assert lib.cuddh_element_lane_tables(4, hD.ctypes.data, hG.ctypes.data, None) == 1
