"""The host side of the lattice sweeps of cd.WaveHoltz (csrc/src/wave_lattice.cpp), through the C handle layer: no GPU.

Kronecker identity: on a uniform rectangle mesh the collocated stiffness and the lumped mass of tests/waveholtz_reference.py are
    K = (hy/hx) diag(Wy) (x) Ax + (hx/hy) Ay (x) diag(Wx),      m = (hx hy / 4) Wy (x) Wx        (lattice index I + Lx J)
with the product's own tables A, w (cuddh_wave_lattice_tables) assembled along a row of elements, through the permutation the
product's map builder returns (cuddh_wave_lattice_map).  Gate 1e-12 of the largest entry, the project's "summation order only"
gate (measured with a coordinate-derived permutation: <= 7.2e-16; through the product's map and tables: K <= 6.3e-16, m <= 4.9e-16).

The map builder accepts uniform rectangles (nx != ny, hx != hy, an offset origin, one element in a direction) and refuses the
unstructured square, a 3 x 3 lattice with one interior vertex moved by 1e-3 h and the same lattice with two elements swapped.
cd.WaveHoltz refuses a bad sweep before it touches the space.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import cuddhelmholtz_amd as cd
from cuddhelmholtz_amd import _native as N

from conftest import GOLDEN

GATE = 1e-12


def lattice_map(fem):
    """(error code, dims {nx, ny, Lx, Ly, stride}, (hx, hy), node_of) of cuddh_wave_lattice_map"""
    dims, h, node_of = np.zeros(5, dtype=np.int32), np.zeros(2), np.full(fem.size(), -7, dtype=np.int32)
    err = N.lib.cuddh_wave_lattice_map(fem._h, dims.ctypes.data, h.ctypes.data, node_of.ctypes.data)
    return err, dict(zip(("nx", "ny", "Lx", "Ly", "stride"), map(int, dims))), (float(h[0]), float(h[1])), node_of


def tables(nb):
    A, w, basis = np.zeros((nb, nb)), np.zeros(nb), cd.Basis(nb)
    N.check_capi(N.lib.cuddh_wave_lattice_tables(basis._h, A.ctypes.data, w.ctypes.data))
    return A, w


def assembled(n, A, w):
    """A and w along a row of n elements that overlap in one node"""
    nb = len(w)
    L = n * (nb - 1) + 1
    Ah, W = np.zeros((L, L)), np.zeros(L)
    for e in range(n):
        s = slice(e * (nb - 1), e * (nb - 1) + nb)
        Ah[s, s] += A
        W[s] += w
    return Ah, W


@functools.lru_cache(maxsize=None)
def space(nx, ny, nb, box):
    ax, bx, ay, by = box
    return cd.H1Space(cd.Mesh2D.uniform_rect(nx, ax, bx, ny, ay, by), cd.Basis(nb))


SQUARE = (-1.0, 1.0, -1.0, 1.0)
IDENTITY_CASES = [(3, 3, 4, SQUARE), (4, 2, 4, (-1.0, 1.0, 0.0, 0.7)), (2, 3, 5, SQUARE), (3, 2, 2, SQUARE), (2, 2, 3, SQUARE)]


def test_tables_are_the_element_matrix_of_the_collocated_rule():
    for nb in range(2, 9):
        A, w = tables(nb)
        assert np.array_equal(A, A.T) or np.abs(A - A.T).max() < 1e-14 * np.abs(A).max()
        assert abs(w.sum() - 2.0) < 1e-14 and np.all(w > 0)
        assert np.abs(A.sum(axis=1)).max() < 1e-12 * np.abs(A).max()  # constants are in the kernel of a stiffness matrix
    A, w = tables(2)
    assert np.allclose(A, [[0.5, -0.5], [-0.5, 0.5]], rtol=0, atol=1e-15) and np.allclose(w, [1.0, 1.0], rtol=0, atol=1e-15)


@pytest.mark.parametrize("nx,ny,nb,box", IDENTITY_CASES, ids=lambda v: str(v) if isinstance(v, int) else "box")
def test_kronecker_identity_through_the_products_map(nx, ny, nb, box):
    import oracle
    import waveholtz_reference as wr

    ax, bx, ay, by = box
    c = wr.Case(oracle.Discretization(oracle.Mesh.uniform_rect(nx, ax, bx, ny, ay, by), nb), 2.0)
    fem = space(nx, ny, nb, box)
    assert fem.size() == c.d.ndof
    err, dims, (hx, hy), node_of = lattice_map(fem)
    assert err == 0, N.last_error()
    assert (dims["nx"], dims["ny"]) == (nx, ny)
    A, w = tables(nb)
    Ax, Wx = assembled(nx, A, w)
    Ay, Wy = assembled(ny, A, w)
    K = (hy / hx) * np.kron(np.diag(Wy), Ax) + (hx / hy) * np.kron(Ay, np.diag(Wx))
    m = 0.25 * hx * hy * np.kron(Wy, Wx)
    K_dof, m_dof = K[np.ix_(node_of, node_of)], m[node_of]
    want_K, want_m = c.K_lobatto, c.mh[0]
    err_K = float(np.abs(K_dof - want_K).max() / np.abs(want_K).max())
    err_m = float(np.abs(m_dof - want_m).max() / np.abs(want_m).max())
    print(f"lattice identity {nx}x{ny} nb{nb}: K {err_K:.2e} m {err_m:.2e}")
    assert err_K < GATE and err_m < GATE


@pytest.mark.parametrize("nx,ny,nb,box", [(3, 2, 4, (-1.0, 1.0, 0.0, 0.7)), (1, 4, 3, (2.0, 3.0, -5.0, -4.2)), (5, 1, 5, (0.25, 4.0, 10.0, 10.5)),
                                          (1, 1, 2, SQUARE), (4, 4, 8, SQUARE), (7, 3, 4, (-3.0, -1.0, 0.5, 0.75))],
                         ids=lambda v: str(v) if isinstance(v, int) else "box")
def test_map_builder_accepts_uniform_rectangles(nx, ny, nb, box):
    fem = space(nx, ny, nb, box)
    err, dims, (hx, hy), node_of = lattice_map(fem)
    assert err == 0, N.last_error()
    H = nb - 1
    Lx, Ly = nx * H + 1, ny * H + 1
    assert dims == {"nx": nx, "ny": ny, "Lx": Lx, "Ly": Ly, "stride": Lx + Lx % 2}
    assert math.isclose(hx, (box[1] - box[0]) / nx, rel_tol=1e-13) and math.isclose(hy, (box[3] - box[2]) / ny, rel_tol=1e-13)
    assert np.array_equal(np.sort(node_of), np.arange(Lx * Ly))  # a bijection
    # consistent with the collocation points: x depends on I alone and grows with it, y on J
    X = fem.physical_coordinates()
    grid = np.empty((2, Ly, Lx))
    grid[:, node_of // Lx, node_of % Lx] = X
    tol = 1e-12 * max(abs(v) for v in box)
    assert np.abs(grid[0] - grid[0][0]).max() <= tol and np.abs(grid[1] - grid[1][:, :1]).max() <= tol
    assert np.all(np.diff(grid[0][0]) > 0) and np.all(np.diff(grid[1][:, 0]) > 0)
    assert math.isclose(grid[0][0][0], box[0], abs_tol=tol) and math.isclose(grid[0][0][-1], box[1], abs_tol=tol)
    assert math.isclose(grid[1][0][0], box[2], abs_tol=tol) and math.isclose(grid[1][-1][0], box[3], abs_tol=tol)
    # the outputs are optional
    assert N.lib.cuddh_wave_lattice_map(fem._h, None, None, None) == 0


def lattice_3x3():
    mesh = cd.Mesh2D.uniform_rect(3, -1.0, 1.0, 3, -1.0, 1.0)
    return mesh.vertices().copy(), mesh.elements().copy()


def refused(mesh, nb=4):
    fem = cd.H1Space(mesh, cd.Basis(nb))
    err, _, _, node_of = lattice_map(fem)
    assert err != 0 and N.last_error().startswith("WaveHoltz error: sweep:"), N.last_error()
    assert np.all(node_of == -7)  # nothing was written
    # and so does the solver's constructor, before it allocates anything (no device here)
    a = np.ones(fem.size())
    h = N.lib.cuddh_waveholtz_create_sweep(1.0, a.ctypes.data, fem._h, 0, 1, 1, 1, None, -1, 1)
    assert not h and N.last_error().startswith("WaveHoltz error: sweep:"), N.last_error()
    with pytest.raises(ValueError, match="WaveHoltz error: sweep:"):
        cd.WaveHoltz(1.0, a, fem, stiffness="lobatto", sweep="lattice")


def test_map_builder_takes_a_copy_of_a_lattice_from_vertices():
    xy, elems = lattice_3x3()
    fem = cd.H1Space(cd.Mesh2D.from_vertices(xy, elems), cd.Basis(4))
    err, dims, _, node_of = lattice_map(fem)
    assert err == 0 and (dims["nx"], dims["ny"]) == (3, 3), N.last_error()
    assert np.array_equal(np.sort(node_of), np.arange(100))


def test_map_builder_refuses_the_unstructured_square():
    refused(cd.Mesh2D.load(GOLDEN / "unstructured_square"))


def test_map_builder_refuses_a_moved_interior_vertex():
    xy, elems = lattice_3x3()
    h = 2.0 / 3.0
    xy[5] += (1e-3 * h, 0.0)  # vertex (1, 1) of the 4 x 4 vertices
    refused(cd.Mesh2D.from_vertices(xy, elems))
    xy, elems = lattice_3x3()
    xy[10] += (0.0, -1e-3 * h)
    refused(cd.Mesh2D.from_vertices(xy, elems), nb=3)


def test_map_builder_refuses_swapped_elements():
    xy, elems = lattice_3x3()
    elems[[1, 5]] = elems[[5, 1]]
    refused(cd.Mesh2D.from_vertices(xy, elems))


def test_native_refusals_of_the_option_itself():
    fem = space(2, 2, 2, SQUARE)
    a = np.ones(fem.size())
    for stiffness, sweep in ((0, 1), (1, 2), (1, -1)):
        h = N.lib.cuddh_waveholtz_create_sweep(1.0, a.ctypes.data, fem._h, 0, 1, 1, stiffness, None, -1, sweep)
        assert not h and N.last_error().startswith("WaveHoltz error: sweep:"), (stiffness, sweep, N.last_error())
    assert N.lib.cuddh_waveholtz_sweep(None) == -1


@pytest.mark.parametrize("kwargs", [dict(sweep="grid"), dict(sweep=1), dict(sweep="lattice", stiffness="gauss"), dict(sweep="lattice")],
                         ids=["grid", "1", "lattice-gauss", "lattice-default-stiffness"])
def test_bad_sweep_raises_before_the_space_is_touched(kwargs):
    class NoSpace:  # anything that touches the space fails the test with another exception
        def __getattr__(self, name):
            raise AssertionError(f"the space was used ({name}) before the arguments were checked")

    with pytest.raises(ValueError, match="sweep"):
        cd.WaveHoltz(1.0, np.ones(4), NoSpace(), **kwargs)
