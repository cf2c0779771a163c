"""DDH with subdomains from element labels, on the CPU: the test-side restatement (tests/ddh_general.py) proven against the
oracle's block form, the general fixed point proven against helmholtz_direct, the product's host tables against both, and
every rejection of DDH.from_labels.  Every distance is printed (`pytest -s`)."""
import math

import numpy as np
import pytest

import ddh_general as dg
import helmholtz_direct as hd
import oracle
from conftest import GOLDEN
from oracle.numbering import ddh_tables
from test_ddh_physics import Case

MESH_DIR = GOLDEN / "unstructured_square"
INT_TABLES = ("B", "gI", "sI", "s_dof", "s_fdof", "s_elems", "elems")
REAL_TABLES = ("D", "m", "gmi", "a", "H", "wh_filter", "cs", "sn")


def block_labels(nx, ny, epd):
    ndx = nx // epd
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    return ((i // epd) + ndx * (j // epd)).reshape(-1).astype(np.int32)


@pytest.mark.parametrize("nb,real", [(2, np.float32), (4, np.float32), (4, np.float64), (8, np.float64)])
def test_restated_tables_equal_ddh_tables_on_blocks(nb, real):
    nx, ny = 16, 8
    om = oracle.Mesh.uniform_rect(nx, -1.0, 1.0, ny, -0.5, 0.5)
    d = oracle.Discretization(om, nb)
    _, Dm = oracle.basis_tables(nb, d.gll_x)
    _, detJ, _ = d.metrics(d.gll_x)
    h_a = 1.0 + 0.3 * np.sin(d.coordinates()[0])
    omega = 2 * math.pi * 1.7
    want = ddh_tables(om, d.I, d.ndof, nx, ny, omega, h_a, d.gll_x, d.gll_w, Dm, detJ, real)
    epd = max(1, 16 // nb)
    got = dg.tables(om, d.I, d.ndof, want.n_domains, block_labels(nx, ny, epd), omega, h_a, d.gll_x, d.gll_w, Dm, detJ, real)
    for k in ("n_domains", "n_lambda", "nt", "mx_dof", "mx_fdof", "mx_elems", "orphan_slots"):
        assert getattr(got, k) == getattr(want, k), k
    assert got.dt == want.dt and got.nel1d == 0
    for k in INT_TABLES:
        assert np.array_equal(getattr(got, k), getattr(want, k)), k
    for k in REAL_TABLES:
        a, b = getattr(got, k), getattr(want, k)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
    print(f"restated DDH tables nb={nb} {np.dtype(real).name}: {want.n_domains} blocks, bitwise equal")


@pytest.mark.parametrize("nx,ny", [(8, 8), (16, 4)])
def test_general_fixed_point_equals_block_fixed_point(nx, ny):
    c = Case(nx, ny)
    t = dg.tables(c.om, c.d.I, c.ndof, (nx // 4) * (ny // 4), block_labels(nx, ny, 4), c.omega, c.h_a, c.d.gll_x, c.d.gll_w,
                  oracle.basis_tables(4, c.d.gll_x)[1], c.d.metrics(c.d.gll_x)[1], np.float64)
    O = dg.OracleDDH(c.d, t.n_domains, block_labels(nx, ny, 4), c.omega, c.h_a, np.float64)
    got = dg.fixed_point(t, O.G, c.ndof, c.f)
    want = c.implied_solution()
    e = hd_rel(got, want)
    print(f"general fixed point vs helmholtz_direct.ddh_fixed_point_solution {nx}x{ny}: {e:.2e}")
    assert e < 1e-12


def hd_rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ------------------------------------------------------------------ product host tables (no device needed)
def _fem(mesh, nb):
    import cuddhelmholtz_amd as cd

    return cd.H1Space(mesh, cd.Basis(nb))


def test_product_block_labels_match_the_block_constructor_host_tables():
    import cuddhelmholtz_amd as cd

    nx = 16
    fem = _fem(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), 4)
    h_a = 1.0 + 0.2 * np.cos(fem.physical_coordinates()[0])
    omega = 2 * math.pi * 1.6
    for prec in ("f32", "f64"):
        A = cd.DDH(omega, h_a, fem, nx, nx, precision=prec)
        B = cd.DDH.from_labels(omega, h_a, fem, block_labels(nx, nx, 4), precision=prec)
        ia, ib = A.info(), B.info()
        assert ib["nel1d"] == 0 and ia["nel1d"] == 4
        for k in ("n_domains", "nt", "n_lambda", "mx_dof", "mx_fdof", "is_f64"):
            assert ia[k] == ib[k], k
        assert ia["dt"] == ib["dt"]
        for name in ("B", "gI", "sI", "D", "m", "gmi", "a", "H", "filter", "cs", "sn"):
            assert A.table(name).tobytes() == B.table(name).tobytes(), name


@pytest.mark.parametrize("times", [1, 2])
def test_product_label_tables_match_the_restatement_on_the_fixture(times):
    import cuddhelmholtz_amd as cd

    mesh = cd.Mesh2D.load(MESH_DIR).refined(times)
    fem = _fem(mesh, 4)
    xy, el = mesh.vertices(), mesh.elements()
    labels = dg.morton_labels(xy[el].mean(axis=1))
    n_domains = int(labels.max()) + 1
    om = oracle.Mesh(xy, el)
    d = oracle.Discretization(om, 4)
    h_a = 1.0 + 0.25 * np.sin(2 * d.coordinates()[0]) * np.cos(d.coordinates()[1])
    omega = 2 * math.pi
    t = dg.tables(om, d.I, d.ndof, n_domains, labels, omega, h_a, d.gll_x, d.gll_w, oracle.basis_tables(4, d.gll_x)[1],
                  d.metrics(d.gll_x)[1], np.float64)
    F = cd.DDH.from_labels(omega, h_a, fem, labels, precision="f64")
    info = F.info()
    assert (info["n_domains"], info["nt"], info["n_lambda"], info["mx_dof"], info["mx_fdof"], info["nel1d"]) == (
        t.n_domains, t.nt, t.n_lambda, t.mx_dof, t.mx_fdof, 0)
    assert info["dt"] == t.dt
    for name, want in (("B", t.B), ("sI", t.sI)):
        assert np.array_equal(F.table(name), want.reshape(-1, order="F")), name
    # gI: equal on every subdomain dof; the padding past a subdomain's size is 0 in the product (a valid index for the
    # gathers that run over all mx_dof * n_domains entries), -1 in the restatement
    gI, want = F.table("gI"), t.gI.reshape(-1, order="F")
    assert np.array_equal(gI[want >= 0], want[want >= 0]) and not gI[want < 0].any()
    e = max(np.max(np.abs(F.table(n) - getattr(t, k).reshape(-1, order="F")) / np.max(np.abs(getattr(t, k))))
            for n, k in (("m", "m"), ("gmi", "gmi"), ("a", "a"), ("H", "H")))
    print(f"fixture x{times} ({mesh.n_elem()} quads, {n_domains} Morton parts): integer tables equal, masses/H/a {e:.1e}")
    assert e < 1e-13


# ------------------------------------------------------------------ rejection, before anything is allocated
@pytest.fixture(scope="module")
def fixture_space():
    import cuddhelmholtz_amd as cd

    mesh = cd.Mesh2D.load(MESH_DIR).refined(1)
    return mesh, _fem(mesh, 4)


def test_rejects_bad_labels(fixture_space):
    import cuddhelmholtz_amd as cd

    mesh, fem = fixture_space
    n = mesh.n_elem()
    h_a = np.ones(fem.size())
    good = dg.morton_labels(mesh.vertices()[mesh.elements()].mean(axis=1))
    with pytest.raises(ValueError, match="labels for"):
        cd.DDH.from_labels(1.0, h_a, fem, good[:-1])
    bad = good.copy()
    bad[3] = -1
    with pytest.raises(ValueError, match="out of range"):
        cd.DDH.from_labels(1.0, h_a, fem, bad)
    empty = good.copy()
    empty[empty >= 2] += 1  # no element has label 2
    with pytest.raises(RuntimeError, match="no elements"):
        cd.DDH.from_labels(1.0, h_a, fem, empty)
    big = good.copy()
    big[big == 1] = 0  # 32 elements of n_basis 4 = 512 element nodes
    with pytest.raises(RuntimeError, match="at most 256"):
        cd.DDH.from_labels(1.0, h_a, fem, big, precision="f64")
    assert n == 476


@pytest.mark.parametrize("kernel", [1, 2, 3, 5, 8, 11])
def test_rejects_block_kernels(fixture_space, kernel):
    import cuddhelmholtz_amd as cd

    mesh, fem = fixture_space
    labels = dg.morton_labels(mesh.vertices()[mesh.elements()].mean(axis=1))
    with pytest.raises(RuntimeError, match="kernel"):
        cd.DDH.from_labels(1.0, np.ones(fem.size()), fem, labels, kernel=kernel)


def test_rejects_kernel9_where_it_does_not_apply(fixture_space):
    import cuddhelmholtz_amd as cd

    mesh, _ = fixture_space
    labels16 = dg.morton_labels(mesh.vertices()[mesh.elements()].mean(axis=1), 16)
    fem3 = _fem(mesh, 3)
    with pytest.raises(RuntimeError, match="kernel 9"):
        cd.DDH.from_labels(1.0, np.ones(fem3.size()), fem3, labels16, kernel=9)
    fem2 = _fem(mesh, 2)
    labels20 = dg.morton_labels(mesh.vertices()[mesh.elements()].mean(axis=1), 20)
    with pytest.raises(RuntimeError, match="kernel 9"):
        cd.DDH.from_labels(1.0, np.ones(fem2.size()), fem2, labels20, kernel=9)
    # the same partitions are fine for kernel 10 / auto
    cd.DDH.from_labels(1.0, np.ones(fem3.size()), fem3, labels16, kernel=10)
    cd.DDH.from_labels(1.0, np.ones(fem2.size()), fem2, labels20)


def test_star_of_vertex_98_is_kept_whole():
    import cuddhelmholtz_amd as cd

    mesh = cd.Mesh2D.load(MESH_DIR).refined(1)
    el = mesh.elements()
    labels = dg.with_whole_star(dg.morton_labels(mesh.vertices()[el].mean(axis=1)), el, 98)
    assert 98 in dg.whole_stars(labels, el)
    assert np.bincount(labels).max() <= 16 and np.bincount(labels).min() >= 1
