"""DDH(..., block=): subdomains of block x block elements instead of the reference's 16 / n_basis per side.  CPU only: the
host tables are built without a device, as in tests/test_host_numbering.py.

  * table identity: n_basis 4, block 8 on 16 x 16 and 24 x 16 elements (rectangular elements, an odd number of subdomains per
    row), f32 and f64: every host table of DDH.table and nt, dt against tests/ddh_general.tables on the labels of 8 x 8
    blocks.  Integer tables identical, real tables with the equality of test_host_numbering.test_ddh_constructor_tables;
  * the default is unchanged: block None, 0 and 16 / n_basis give bitwise the tables of the constructor without block;
  * refusals, each with a message that names the limit: more than 1024 element nodes, nx no multiple of block, block < 0;
    the largest accepted shapes are accepted.
"""
import math

import numpy as np
import pytest

import cuddhelmholtz_amd as cd
import ddh_general as dg
import oracle

INT_TABLES = ("B", "gI", "sI")
REAL_TABLES = ("m", "gmi", "a", "H", "filter", "cs", "sn")


def block_labels(nx, ny, block):
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    return ((i // block) + (nx // block) * (j // block)).reshape(-1).astype(np.int32)


def product(nx, ny, nb, h_a, omega, precision="f32", **kw):
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, ny, -1.0, 1.0), cd.Basis(nb))
    return cd.DDH(omega, h_a, fem, nx, ny, precision=precision, **kw)


@pytest.mark.parametrize("nx,ny", [(16, 16), (24, 16)])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_block_8_tables_are_those_of_8x8_block_labels(nx, ny, precision):
    nb, block = 4, 8
    omega = 2 * math.pi * nx / 10
    om = oracle.Mesh.uniform_rect(nx, -1.0, 1.0, ny, -1.0, 1.0)
    d = oracle.Discretization(om, nb)
    h_a = 0.5 + np.random.default_rng(3).random(d.ndof)
    real = np.float32 if precision == "f32" else np.float64
    n_domains = (nx // block) * (ny // block)
    t = dg.tables(om, d.I, d.ndof, n_domains, block_labels(nx, ny, block), omega, h_a, d.gll_x, d.gll_w, oracle.basis_tables(nb, d.gll_x)[1],
                  d.metrics(d.gll_x)[1], real)
    F = product(nx, ny, nb, h_a, omega, precision, block=block)
    info = F.info()
    assert F.size() == 2 * t.n_lambda
    assert (info["n_domains"], info["nt"], info["n_lambda"], info["mx_dof"], info["mx_fdof"], info["nel1d"]) == (
        n_domains, t.nt, t.n_lambda, t.mx_dof, t.mx_fdof, block)
    assert (t.mx_dof, t.mx_fdof, t.mx_elems) == (25 * 25, 4 * 24, 64)
    assert abs(info["dt"] - t.dt) < 1e-18
    refs = {"B": t.B, "gI": t.gI, "sI": t.sI, "m": t.m, "gmi": t.gmi, "a": t.a, "H": t.H, "filter": t.wh_filter, "cs": t.cs, "sn": t.sn}
    for name in INT_TABLES:
        assert np.array_equal(F.table(name), refs[name].reshape(-1, order="F")), name
    rtol = 2e-7 if precision == "f32" else 1e-13
    for name in REAL_TABLES:
        got, ref = F.table(name), refs[name].reshape(-1, order="F")
        assert got.dtype == real
        assert np.allclose(got, ref, rtol=rtol, atol=rtol * np.abs(ref).max()), name


@pytest.mark.parametrize("nb,nx", [(4, 8), (8, 4), (5, 6)])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_default_block_is_unchanged(nb, nx, precision):
    omega = 2 * math.pi * nx / 10
    h_a = 0.5 + np.random.default_rng(5).random((nx * (nb - 1) + 1) ** 2)
    today = product(nx, nx, nb, h_a, omega, precision)
    default = max(1, 16 // nb)
    for block in (None, 0, default):
        F = product(nx, nx, nb, h_a, omega, precision, block=block)
        assert F.size() == today.size()
        a, b = F.info(), today.info()
        assert a == b and a["nel1d"] == default
        for name in INT_TABLES + ("D",) + REAL_TABLES:
            x, y = F.table(name), today.table(name)
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), (block, name)


def test_refusals_and_the_largest_accepted_shapes():
    def build(nb, nx, block, precision="f32"):
        return product(nx, nx, nb, np.ones((nx * (nb - 1) + 1) ** 2), 2.0, precision, block=block)

    with pytest.raises(RuntimeError, match="1024"):
        build(4, 18, 9)  # 16 * 81 = 1,296 element nodes
    with pytest.raises(RuntimeError, match="multiples of block = 8"):
        build(4, 20, 8)
    with pytest.raises(RuntimeError, match="at least 1"):
        build(4, 8, -1)
    with pytest.raises(RuntimeError, match="1024"):
        build(8, 10, 5)  # 64 * 25 = 1,600
    for precision in ("f32", "f64"):
        F = build(8, 8, 4, precision)  # 64 * 16 = 1,024: accepted
        assert (F.info()["nel1d"], F.info()["n_domains"], F.info()["mx_dof"]) == (4, 4, 29 * 29)
        F = build(4, 16, 8, precision)  # 16 * 64 = 1,024
        assert (F.info()["nel1d"], F.info()["n_domains"]) == (8, 4)
    F = build(5, 12, 6)  # 25 * 36 = 900
    assert (F.info()["nel1d"], F.info()["n_domains"], F.info()["mx_dof"]) == (6, 4, 25 * 25)
    F = build(4, 6, 1)  # one element per subdomain
    assert (F.info()["nel1d"], F.info()["n_domains"]) == (1, 36)
