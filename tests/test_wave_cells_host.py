"""The host side of the lattice sweeps on grid meshes with missing cells (csrc/src/wave_lattice.cpp: build_wave_cells_map;
csrc/src/meshio.cpp: grid_cells), through the C handle layer: no GPU.

A grid mesh with missing cells is a subset of the cells of a uniform nx x ny grid in ascending cell index (cd.Mesh2D.grid_cells).
cuddh_wave_lattice_map_cells returns the grid, the cell flags and dof -> lattice node; the map is an injection whose image is the
nodes of the existing cells.

The identity: with A, w from cuddh_wave_lattice_tables, the stencil stated at the head of csrc/kernels/wave_cells.hip (per node:
sL, sR, sB, sA and the four flags) written out as a dense matrix on the lattice and restricted to the image of the map is
tests/waveholtz_reference.py's K_lobatto, and the per-cell sum of (hx hy / 4) w (x) w is its lumped mass.  Gate 1e-12 of the largest
entry, the "summation order only" gate of tests/test_wave_lattice_host.py.

Refused, with nothing written: cells out of order, a duplicated cell, a moved vertex, a cell of another size, the unstructured
square.  cuddh_wave_lattice_map keeps refusing a mesh with a hole; launch="pair" on such a mesh is a ValueError.
"""
import functools

import numpy as np
import pytest

import cuddhelmholtz_amd as cd
from cuddhelmholtz_amd import _native as N

from conftest import GOLDEN

GATE = 1e-12
SQUARE = (-1.0, 1.0, -1.0, 1.0)


def mask(nx, ny, *holes):
    """(ny, nx) bools, false in the half-open cell boxes (i0, j0, i1, j1)"""
    present = np.ones((ny, nx), dtype=bool)
    for i0, j0, i1, j1 in holes:
        present[j0:j1, i0:i1] = False
    return present


MESHES = {
    # name: (nx, ny, box, holes)
    "L": (6, 6, SQUARE, [(3, 3, 6, 6)]),
    "hole": (7, 5, (-1.0, 2.5, 0.0, 1.0), [(2, 1, 4, 3)]),
    "notch": (5, 4, SQUARE, [(2, 0, 3, 2)]),
    "two-holes": (8, 5, (0.25, 4.0, 10.0, 10.5), [(1, 1, 2, 3), (5, 2, 7, 4)]),
    "row": (5, 1, (2.0, 3.0, -5.0, -4.2), []),
    "corner-touch": (4, 4, SQUARE, [(1, 1, 2, 2), (2, 2, 3, 3)]),
    "staircase": (4, 3, SQUARE, [(0, 1, 1, 3), (1, 2, 2, 3), (3, 0, 4, 1)]),
}


@functools.lru_cache(maxsize=None)
def space(name, nb):
    nx, ny, (ax, bx, ay, by), holes = MESHES[name]
    present = mask(nx, ny, *holes)
    mesh = cd.Mesh2D.grid_cells(nx, ax, bx, ny, ay, by, present)
    return mesh, cd.H1Space(mesh, cd.Basis(nb)), present


def cells_map(fem, n_cells=4096):
    """(error code, dims, (hx, hy), node_of, cell bytes) of cuddh_wave_lattice_map_cells; -7 / 7 where nothing was written"""
    dims, h, node_of = np.zeros(5, dtype=np.int32), np.zeros(2), np.full(fem.size(), -7, dtype=np.int32)
    cell = np.full(n_cells, 7, dtype=np.uint8)
    err = N.lib.cuddh_wave_lattice_map_cells(fem._h, dims.ctypes.data, h.ctypes.data, node_of.ctypes.data, cell.ctypes.data)
    return err, dict(zip(("nx", "ny", "Lx", "Ly", "stride"), map(int, dims))), (float(h[0]), float(h[1])), node_of, cell


def tables(nb):
    A, w, basis = np.zeros((nb, nb)), np.zeros(nb), cd.Basis(nb)
    N.check_capi(N.lib.cuddh_wave_lattice_tables(basis._h, A.ctypes.data, w.ctypes.data))
    return A, w


def nodes_of_cells(present, nb):
    """the lattice nodes I + Lx J that lie in an existing cell"""
    H = nb - 1
    ny, nx = present.shape
    Lx = nx * H + 1
    nodes = set()
    for j, i in zip(*np.nonzero(present)):
        for b in range(nb):
            for a in range(nb):
                nodes.add(i * H + a + Lx * (j * H + b))
    return np.array(sorted(nodes))


def stencil_matrix(present, nb, A, w, cx, cy):
    """K of the header of wave_cells.hip as a dense matrix on the whole lattice: row (I, J) from sL, sR, sB, sA and the four flags"""
    H = nb - 1
    ny, nx = present.shape
    Lx, Ly = nx * H + 1, ny * H + 1
    flag = lambda a, b: 1.0 if 0 <= a < nx and 0 <= b < ny and present[b, a] else 0.0  # noqa: E731

    def sums(i):
        """[(cell index offset, weight, {d: coefficient})] of the one or two sums of a node at position i of a line"""
        k = i % H
        if k:
            return [(i // H, w[k], {j - k: A[k, j] for j in range(nb)})]
        return [(i // H - 1, w[H], {j - H: A[H, j] for j in range(nb)}), (i // H, w[0], {j: A[0, j] for j in range(nb)})]

    K = np.zeros((Lx * Ly, Lx * Ly))
    for J in range(Ly):
        for I in range(Lx):
            row = K[I + Lx * J]
            for a, wx, sx in sums(I):
                for b, wy, sy in sums(J):
                    f = flag(a, b)
                    if f == 0.0:
                        continue
                    for d, coef in sx.items():
                        row[I + d + Lx * J] += cx * wy * f * coef
                    for d, coef in sy.items():
                        row[I + Lx * (J + d)] += cy * wx * f * coef
    return K


CASES = [("L", 4), ("hole", 4), ("notch", 5), ("two-holes", 2), ("row", 5), ("corner-touch", 3), ("staircase", 8), ("hole", 8), ("L", 2)]


@pytest.mark.parametrize("name,nb", CASES)
def test_map_builder_accepts_grids_with_missing_cells(name, nb):
    nx, ny, box, _ = MESHES[name]
    mesh, fem, present = space(name, nb)
    assert mesh.n_elem() == int(present.sum())
    err, dims, (hx, hy), node_of, cell = cells_map(fem)
    assert err == 0, N.last_error()
    H = nb - 1
    Lx, Ly = nx * H + 1, ny * H + 1
    assert dims == {"nx": nx, "ny": ny, "Lx": Lx, "Ly": Ly, "stride": Lx + Lx % 2}
    assert np.isclose(hx, (box[1] - box[0]) / nx, rtol=1e-13) and np.isclose(hy, (box[3] - box[2]) / ny, rtol=1e-13)
    assert np.array_equal(cell[: nx * ny].reshape(ny, nx), present.astype(np.uint8)) and np.all(cell[nx * ny:] == 7)
    # an injection whose image is exactly the nodes of the existing cells
    assert np.array_equal(np.sort(node_of), nodes_of_cells(present, nb))
    # consistent with the collocation points: x depends on I alone and grows with it, y on J
    X = fem.physical_coordinates()
    grid = np.full((2, Ly, Lx), np.nan)
    grid[:, node_of // Lx, node_of % Lx] = X
    tol = 1e-12 * max(abs(v) for v in box)
    xs, ys = np.nanmin(grid[0], axis=0), np.nanmin(grid[1], axis=1)
    assert np.nanmax(np.abs(grid[0] - xs[None, :])) <= tol and np.nanmax(np.abs(grid[1] - ys[:, None])) <= tol
    assert np.all(np.diff(xs) > 0) and np.all(np.diff(ys) > 0)
    assert abs(xs[0] - box[0]) <= tol and abs(xs[-1] - box[1]) <= tol and abs(ys[0] - box[2]) <= tol and abs(ys[-1] - box[3]) <= tol
    # the outputs are optional
    assert N.lib.cuddh_wave_lattice_map_cells(fem._h, None, None, None, None) == 0


@pytest.mark.parametrize("name,nb", [("L", 4), ("hole", 3), ("notch", 5), ("corner-touch", 2), ("staircase", 4)])
def test_stencil_identity_through_the_products_map(name, nb):
    import oracle
    import waveholtz_reference as wr

    mesh, fem, present = space(name, nb)
    c = wr.Case(oracle.Discretization(oracle.Mesh(mesh.vertices(), mesh.elements()), nb), 2.0)
    assert fem.size() == c.d.ndof
    err, dims, (hx, hy), node_of, _ = cells_map(fem)
    assert err == 0, N.last_error()
    A, w = tables(nb)
    K = stencil_matrix(present, nb, A, w, hy / hx, hx / hy)
    H, Lx, Ly = nb - 1, dims["Lx"], dims["Ly"]
    m = np.zeros((Ly, Lx))
    for j, i in zip(*np.nonzero(present)):
        m[j * H: j * H + nb, i * H: i * H + nb] += 0.25 * hx * hy * np.outer(w, w)
    m = m.reshape(-1)
    void = np.setdiff1d(np.arange(Lx * Ly), node_of)
    assert not K[void].any() and not K[:, void].any() and not m[void].any()  # a void node has a zero row, a zero column and no mass
    want_K, want_m = c.K_lobatto, c.mh[0]
    err_K = float(np.abs(K[np.ix_(node_of, node_of)] - want_K).max() / np.abs(want_K).max())
    err_m = float(np.abs(m[node_of] - want_m).max() / np.abs(want_m).max())
    print(f"cells identity {name} nb{nb}: ndof={c.d.ndof} K {err_K:.2e} m {err_m:.2e}")
    assert err_K < GATE and err_m < GATE


def test_a_full_grid_through_grid_cells_is_the_uniform_rectangle():
    full = cd.Mesh2D.grid_cells(4, -1.0, 1.0, 3, 0.0, 0.7, np.ones((3, 4), dtype=bool))
    rect = cd.Mesh2D.uniform_rect(4, -1.0, 1.0, 3, 0.0, 0.7)
    assert np.array_equal(full.vertices(), rect.vertices()) and np.array_equal(full.elements(), rect.elements())
    fem = cd.H1Space(full, cd.Basis(4))
    node_of = np.zeros(fem.size(), dtype=np.int32)
    assert N.lib.cuddh_wave_lattice_map(fem._h, None, None, node_of.ctypes.data) == 0, N.last_error()  # the full detection takes it
    err, dims, _, node_of_cells, cell = cells_map(fem)
    assert err == 0 and np.array_equal(node_of_cells, node_of) and np.all(cell[:12] == 1)


def grid_3x3():
    mesh = cd.Mesh2D.uniform_rect(3, -1.0, 1.0, 3, -1.0, 1.0)
    return mesh.vertices().copy(), mesh.elements().copy()


def refused(mesh, nb=4):
    fem = cd.H1Space(mesh, cd.Basis(nb))
    err, dims, h, node_of, cell = cells_map(fem)
    assert err != 0 and N.last_error().startswith("WaveHoltz error: sweep:"), N.last_error()
    assert np.all(node_of == -7) and np.all(cell == 7) and not any(dims.values()) and h == (0.0, 0.0)  # nothing was written
    a = np.ones(fem.size())
    with pytest.raises(ValueError, match="WaveHoltz error: sweep:"):
        cd.WaveHoltz(1.0, a, fem, stiffness="lobatto", sweep="lattice")


def test_refuses_cells_out_of_order():
    xy, elems = grid_3x3()
    elems[[1, 5]] = elems[[5, 1]]
    refused(cd.Mesh2D.from_vertices(xy, elems))
    xy, elems = grid_3x3()
    refused(cd.Mesh2D.from_vertices(xy, elems[[0, 1, 2, 3, 5, 4, 6, 7, 8]]), nb=3)  # also with a cell missing
    refused(cd.Mesh2D.from_vertices(xy, elems[[0, 2, 1, 8]]), nb=2)


def test_refuses_a_duplicated_cell():
    xy, elems = grid_3x3()
    xy2 = np.concatenate([xy, xy[elems[4]]])  # a second copy of cell 4 on vertices of its own
    elems2 = np.concatenate([elems[:5], [[16, 17, 18, 19]], elems[5:]]).astype(np.int32)
    refused(cd.Mesh2D.from_vertices(xy2, elems2))


def test_refuses_a_moved_vertex():
    h = 2.0 / 3.0
    xy, elems = grid_3x3()
    xy[5] += (1e-3 * h, 0.0)
    refused(cd.Mesh2D.from_vertices(xy, elems))
    xy, elems = grid_3x3()
    xy[10] += (0.0, -1e-3 * h)
    refused(cd.Mesh2D.from_vertices(xy, np.delete(elems, 0, axis=0)), nb=3)


def test_refuses_a_cell_of_another_size():
    # two cells side by side, the second twice as wide
    xy = np.array([[0.0, 0.0], [1.0, 0.0], [3.0, 0.0], [0.0, 1.0], [1.0, 1.0], [3.0, 1.0]])
    elems = np.array([[0, 1, 4, 3], [1, 2, 5, 4]], dtype=np.int32)
    refused(cd.Mesh2D.from_vertices(xy, elems))
    # a grid whose last column is 1.5 cells wide
    xy = np.array([[0.0, 0.0], [1.0, 0.0], [2.5, 0.0], [0.0, 1.0], [1.0, 1.0], [2.5, 1.0]])
    refused(cd.Mesh2D.from_vertices(xy, elems), nb=3)


def test_refuses_the_unstructured_square():
    refused(cd.Mesh2D.load(GOLDEN / "unstructured_square"))


def test_the_full_detection_still_refuses_a_hole_and_pair_launches_are_refused():
    _, fem, _ = space("hole", 4)
    node_of = np.full(fem.size(), -7, dtype=np.int32)
    err = N.lib.cuddh_wave_lattice_map(fem._h, None, None, node_of.ctypes.data)
    assert err != 0 and N.last_error().startswith("WaveHoltz error: sweep:") and np.all(node_of == -7), N.last_error()
    a = np.ones(fem.size())
    for precision in ("f64", "f32"):
        with pytest.raises(ValueError, match="WaveHoltz error: launch:"):
            cd.WaveHoltz(1.0, a, fem, stiffness="lobatto", sweep="lattice", launch="pair", precision=precision)
    h = N.lib.cuddh_waveholtz_create_launch(1.0, a.ctypes.data, fem._h, 0, 1, 1, 1, None, -1, 1, 0, 1)
    assert not h and N.last_error().startswith("WaveHoltz error: launch:") and "cells" in N.last_error(), N.last_error()


def test_grid_cells_refuses_bad_masks():
    with pytest.raises(ValueError, match="at least one"):
        cd.Mesh2D.grid_cells(3, 0.0, 1.0, 2, 0.0, 1.0, np.zeros((2, 3), dtype=bool))
    for bad in (np.ones((3, 2), dtype=bool), np.ones(6, dtype=bool), np.ones((2, 3, 1), dtype=bool)):
        with pytest.raises(ValueError, match="shape"):
            cd.Mesh2D.grid_cells(3, 0.0, 1.0, 2, 0.0, 1.0, bad)
    assert not N.lib.cuddh_mesh_grid_cells(3, 0.0, 1.0, 2, 0.0, 1.0, np.zeros(6, dtype=np.uint8).ctypes.data)
    assert "grid_cells" in N.last_error()


def test_the_cell_entry_points_are_declared():
    declared = set(N.declared_symbols())
    stages = ("rk2_a", "rk2_b", "rk4_1", "rk4_2", "rk4_3", "rk4_4")
    want = {f"cuddh_hip_wave_cells_{s}_f64" for s in stages} | {f"cuddh_hip_wave_cells32_{s}" for s in stages}
    assert {s for s in declared if s.startswith("cuddh_hip_wave_cells")} == want
    assert {"cuddh_wave_lattice_map_cells", "cuddh_mesh_grid_cells"} <= declared
