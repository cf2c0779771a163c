"""The host side of the lattice sweeps with a per-cell stiffness coefficient (csrc/src/wave_lattice.cpp:
wave_lattice_cell_weights, wave_coefficient_ratio; the cell_stiffness keyword of cd.WaveHoltz), through the C handle layer: no GPU.

The helper tests/wave_weights_reference.py builds the dense K_beta = sum_e beta_e P_e^T K_el P_e from the product's 1-D tables and
the space's element node lists.  It is pinned first: at beta == 1 it is tests/waveholtz_reference.py's K_lobatto to 1e-12 of the
largest entry (the "summation order only" gate of tests/test_wave_cells_host.py), it is symmetric with the constants in its null
space, and beta == c gives c K.

The identity: the weighted stencil stated at the head of csrc/kernels/wave_weights.hip (per node: sL, sR, sB, sA and the four
weights f_XY), written out as a dense matrix on the lattice with the product's tables and restricted by node_of, is K_beta to
1e-12: full 3 x 2, the hole, the notch and the staircase at n_basis 2, 3, 4, 5, 8, beta random in [0.25, 4], and one mesh with a
jump of 100 across a cell edge.

The cell-weight map (cuddh_wave_lattice_cell_weights), the ratio rule (cuddh_waveholtz_coefficient_ratio) on hand-made (a, beta),
and the refusals of Python and of the C API, which come before the space is touched or anything is allocated.
"""
import functools

import numpy as np
import pytest

import cuddhelmholtz_amd as cd
from cuddhelmholtz_amd import _native as N

import wave_weights_reference as ww
from conftest import GOLDEN
from test_wave_cells_host import MESHES, cells_map, mask, space, tables

GATE = 1e-12
STAGES = ("rk2_a", "rk2_b", "rk4_1", "rk4_2", "rk4_3", "rk4_4")


@functools.lru_cache(maxsize=None)
def full_space(nx, ny, box, nb):
    mesh = cd.Mesh2D.uniform_rect(nx, box[0], box[1], ny, box[2], box[3])
    return mesh, cd.H1Space(mesh, cd.Basis(nb)), np.ones((ny, nx), dtype=bool)


def any_space(name, nb):
    if name == "full-3x3":
        return full_space(3, 3, (-1.0, 1.0, -1.0, 1.0), nb)
    if name == "full-3x2":
        return full_space(3, 2, (0.5, 2.0, -1.0, -0.2), nb)
    return space(name, nb)


def lattice_of(fem):
    """(dims, (hx, hy), node_of) of the detection WaveHoltz uses; a full rectangle is a grid with every cell"""
    err, dims, h, node_of, _ = cells_map(fem)
    assert err == 0, N.last_error()
    return dims, h, node_of


def cell_grid(present, beta):
    """(ny, nx) weights: the present cells in ascending order take beta in element order, absent cells 0"""
    grid = np.zeros(present.shape)
    grid[present] = beta  # boolean assignment runs in C order: ascending a + nx b
    return grid


def weighted_stencil_matrix(grid, nb, A, w, cx, cy):
    """K of the header of wave_weights.hip as a dense matrix on the whole lattice: row (I, J) from sL, sR, sB, sA, each pair of a
    column sum and a row sum with the weight f_XY of the cell they meet in"""
    H = nb - 1
    ny, nx = grid.shape
    Lx, Ly = nx * H + 1, ny * H + 1
    weight = lambda a, b: grid[b, a] if 0 <= a < nx and 0 <= b < ny else 0.0  # noqa: E731

    def sums(i):
        """[(cell index, rule weight, {d: coefficient})] of the one or two sums of a node at position i of a line"""
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
                    f = weight(a, b)
                    for d, coef in sx.items():
                        if 0 <= I + d < Lx:
                            row[I + d + Lx * J] += cx * wy * f * coef
                    for d, coef in sy.items():
                        if 0 <= J + d < Ly:
                            row[I + Lx * (J + d)] += cy * wx * f * coef
    return K


# ------------------------------------------------------------------ the helper, pinned
@pytest.mark.parametrize("name,nb", [("full-3x3", 4), ("L", 4), ("hole", 3), ("hole", 4)])
def test_the_helper_at_beta_one_is_the_collocated_stiffness(name, nb):
    import oracle
    import waveholtz_reference as wr

    mesh, fem, present = any_space(name, nb)
    c = wr.Case(oracle.Discretization(oracle.Mesh(mesh.vertices(), mesh.elements()), nb), 2.0)
    assert fem.size() == c.d.ndof
    _, (hx, hy), _ = lattice_of(fem)
    n_elem = mesh.n_elem()
    K1 = ww.weighted_stiffness(fem, hx, hy, np.ones(n_elem))
    scale = np.abs(c.K_lobatto).max()
    err = float(np.abs(K1 - c.K_lobatto).max() / scale)
    print(f"weighted helper at beta = 1, {name} nb{nb}: {err:.2e} of the largest entry")
    assert err < GATE
    beta = np.random.default_rng(3).uniform(0.25, 4.0, n_elem)
    Kb = ww.weighted_stiffness(fem, hx, hy, beta)
    assert np.abs(Kb - Kb.T).max() < GATE * scale and np.abs(Kb @ np.ones(fem.size())).max() < 1e-11 * scale
    assert np.abs(ww.weighted_stiffness(fem, hx, hy, np.full(n_elem, 2.5)) - 2.5 * K1).max() < GATE * scale
    assert np.abs(Kb - K1).max() > 0.1 * scale  # beta matters


# ------------------------------------------------------------------ the stencil identity
def jump_beta(present):
    """1 left of the middle cell column, 100 from it on: a jump of 100 across a cell edge"""
    ny, nx = present.shape
    grid = np.ones((ny, nx))
    grid[:, nx // 2:] = 100.0
    return grid[present]


@pytest.mark.parametrize("nb", [2, 3, 4, 5, 8])
@pytest.mark.parametrize("name", ["full-3x2", "hole", "notch", "staircase", "hole-jump"])
def test_weighted_stencil_identity(name, nb):
    mesh, fem, present = any_space("hole" if name == "hole-jump" else name, nb)
    dims, (hx, hy), node_of = lattice_of(fem)
    n_elem = mesh.n_elem()
    beta = jump_beta(present) if name == "hole-jump" else np.random.default_rng(10 * nb + len(name)).uniform(0.25, 4.0, n_elem)
    A, w = tables(nb)
    K = weighted_stencil_matrix(cell_grid(present, beta), nb, A, w, hy / hx, hx / hy)
    want = ww.weighted_stiffness(fem, hx, hy, beta)
    void = np.setdiff1d(np.arange(dims["Lx"] * dims["Ly"]), node_of)
    assert not K[void].any() and not K[:, void].any()  # a node with no cell around it has a zero row and a zero column
    err = float(np.abs(K[np.ix_(node_of, node_of)] - want).max() / np.abs(want).max())
    print(f"weighted stencil identity {name} nb{nb}: ndof={fem.size()} beta in [{beta.min():.3g}, {beta.max():.3g}] K {err:.2e}")
    assert err < GATE


# ------------------------------------------------------------------ the cell-weight map
def cell_weights(fem, beta, n_cells=512):
    out, dims = np.full(n_cells, -7.0), np.full(2, -7, dtype=np.int32)
    beta = None if beta is None else np.ascontiguousarray(beta, dtype=np.float64)
    err = N.lib.cuddh_wave_lattice_cell_weights(fem._h, None if beta is None else beta.ctypes.data, out.ctypes.data, dims.ctypes.data)
    return err, out, dims


@pytest.mark.parametrize("name,nb", [("full-3x2", 3), ("full-3x3", 4), ("hole", 4), ("two-holes", 2), ("staircase", 5), ("row", 3)])
def test_cell_weight_map(name, nb):
    mesh, fem, present = any_space(name, nb)
    ny, nx = present.shape
    beta = np.random.default_rng(nb).uniform(0.5, 2.0, mesh.n_elem())
    err, out, dims = cell_weights(fem, beta)
    assert err == 0, N.last_error()
    assert tuple(dims) == (nx, ny)
    assert np.array_equal(out[: nx * ny].reshape(ny, nx), cell_grid(present, beta)) and np.all(out[nx * ny:] == -7.0)
    assert np.all(out[: nx * ny].reshape(ny, nx)[~present] == 0.0) and np.all(out[: nx * ny].reshape(ny, nx)[present] > 0.0)
    if present.all():
        assert np.array_equal(out[: nx * ny], beta)  # element e is cell e
    assert N.lib.cuddh_wave_lattice_cell_weights(fem._h, beta.ctypes.data, None, None) == 0  # the outputs are optional


def test_cell_weight_map_refusals_write_nothing():
    mesh, fem, _ = any_space("hole", 4)
    good = np.ones(mesh.n_elem())
    for bad in (None, np.where(np.arange(good.size) == 3, np.nan, good), np.where(np.arange(good.size) == 0, 0.0, good),
                np.where(np.arange(good.size) == good.size - 1, -1.0, good), np.where(np.arange(good.size) == 5, np.inf, good)):
        err, out, dims = cell_weights(fem, bad)
        assert err != 0 and N.last_error().startswith("WaveHoltz error: cell_stiffness:"), N.last_error()
        assert np.all(out == -7.0) and np.all(dims == -7)
    rough = cd.H1Space(cd.Mesh2D.load(GOLDEN / "unstructured_square"), cd.Basis(3))
    err, out, dims = cell_weights(rough, np.ones(rough.mesh.n_elem()))
    assert err != 0 and N.last_error().startswith("WaveHoltz error: sweep:"), N.last_error()
    assert np.all(out == -7.0) and np.all(dims == -7)


# ------------------------------------------------------------------ the ratio rule
def ratio(I, a, beta):
    I = np.asfortranarray(I, dtype=np.int32)  # (nodes per element, n_elem)
    a = np.ascontiguousarray(a, dtype=np.float64)
    beta = None if beta is None else np.ascontiguousarray(beta, dtype=np.float64)
    out = np.full(1, -7, dtype=np.int32)
    err = N.lib.cuddh_waveholtz_coefficient_ratio(I.shape[1], I.shape[0], I.ctypes.data, a.ctypes.data, None if beta is None else beta.ctypes.data,
                                                  out.ctypes.data)
    return err, int(out[0])


def test_ratio_rule():
    import waveholtz_reference as wr

    # three elements of four nodes on eight dofs; the smallest a (0.3) lies in element 1 only
    I = np.array([[0, 1, 2, 3], [2, 3, 4, 5], [5, 6, 7, 0]]).T
    a = np.array([1.0, 0.9, 0.8, 0.7, 0.3, 0.6, 1.2, 2.0])
    one = np.ones(3)
    base = wr.coefficient_ratio(a)
    assert base == 4
    assert ratio(I, a, None) == (0, base) and ratio(I, a, one) == (0, base)
    assert ww.beta_ratio(a, I, one) == base
    # beta = 4 on the cell with the smallest a doubles the speed there: ceil(2 / 0.3) = 7
    beta = np.array([1.0, 4.0, 1.0])
    assert ratio(I, a, beta) == (0, 7) == (0, ww.beta_ratio(a, I, beta))
    # beta = 4 elsewhere: element 0 has min a = 0.7, sqrt(4) / 0.7 = 2.86 < 1 / 0.3
    assert ratio(I, a, np.array([4.0, 1.0, 1.0])) == (0, base)
    # a slow medium: never below 1
    assert ratio(I, 3.0 * a, np.array([0.25, 0.25, 0.25])) == (0, 1)
    # the guard at an exact integer: sqrt(9) / 0.5 = 6 exactly stays 6, not 7; a hair above goes up
    half = np.full(8, 0.5)
    assert ratio(I, half, np.array([1.0, 9.0, 1.0])) == (0, 6)
    assert ratio(I, half, np.array([1.0, 9.0 * (1 + 1e-8), 1.0])) == (0, 7)
    assert ratio(I, half, np.array([1.0, 9.0 * (1 + 1e-10), 1.0])) == (0, 6)  # inside the guard
    assert ratio(I, half, None) == (0, 2) == (0, wr.coefficient_ratio(half))
    # above the maximum of 256: refused, nothing written
    err, out = ratio(I, half, np.array([1.0, 129.0 ** 2, 1.0]))
    assert err != 0 and out == -7 and N.last_error().startswith("WaveHoltz error: time step:"), N.last_error()
    assert ratio(I, half, np.array([1.0, 128.0 ** 2, 1.0])) == (0, 256)
    err, out = ratio(I, a, np.array([1.0, -4.0, 1.0]))
    assert err != 0 and out == -7 and N.last_error().startswith("WaveHoltz error: cell_stiffness:"), N.last_error()


# ------------------------------------------------------------------ refusals
class NoSpace:  # anything that touches the space fails the test with another exception
    def __getattr__(self, name):
        raise AssertionError(f"the space was used ({name}) before the arguments were checked")


@pytest.mark.parametrize("kwargs,match", [
    (dict(cell_stiffness=np.ones(4), sweep="operator", stiffness="lobatto"), "cell_stiffness"),
    (dict(cell_stiffness=np.ones(4)), "cell_stiffness"),
    (dict(cell_stiffness=np.ones(4), sweep="lattice", stiffness="lobatto", launch="pair"), "launch"),
    (dict(cell_stiffness=np.array([1.0, np.nan, 1.0, 1.0]), sweep="lattice", stiffness="lobatto"), "finite and positive"),
    (dict(cell_stiffness=np.array([1.0, np.inf, 1.0, 1.0]), sweep="lattice", stiffness="lobatto"), "finite and positive"),
    (dict(cell_stiffness=np.array([1.0, 0.0, 1.0, 1.0]), sweep="lattice", stiffness="lobatto"), "finite and positive"),
    (dict(cell_stiffness=np.array([1.0, 2.0, -1.0, 1.0]), sweep="lattice", stiffness="lobatto"), "finite and positive"),
    (dict(cell_stiffness=np.ones((2, 2)), sweep="lattice", stiffness="lobatto"), "one-dimensional"),
    (dict(cell_stiffness=1.0, sweep="lattice", stiffness="lobatto"), "one-dimensional"),
    (dict(cell_stiffness="soft", sweep="lattice", stiffness="lobatto"), "cell_stiffness"),
])
def test_python_refuses_before_touching_the_space(kwargs, match):
    with pytest.raises(ValueError, match=match):
        cd.WaveHoltz(1.0, np.ones(4), NoSpace(), **kwargs)


def test_python_refuses_a_wrong_length():
    mesh, fem, _ = any_space("hole", 4)
    a = np.ones(fem.size())
    for n in (mesh.n_elem() - 1, mesh.n_elem() + 1, 35, 0):  # 35: the cells of the grid, not the elements of the mesh
        with pytest.raises(ValueError, match="cell_stiffness values for"):
            cd.WaveHoltz(1.0, a, fem, stiffness="lobatto", sweep="lattice", cell_stiffness=np.ones(n))


def test_native_refusals_carry_their_prefixes():
    mesh, fem, _ = any_space("hole", 4)
    a, beta = np.ones(fem.size()), np.ones(mesh.n_elem())
    create = N.lib.cuddh_waveholtz_create_cell_stiffness

    def refused(prefix, beta_ptr, sweep=1, precision=0, launch=0, ratio=1, coefficient=a):
        h = create(1.0, coefficient.ctypes.data, fem._h, 0, 1, ratio, 1, None, -1, sweep, precision, launch, beta_ptr)
        assert not h and N.last_error().startswith(prefix), N.last_error()

    refused("WaveHoltz error: cell_stiffness:", None)
    for k, v in ((0, np.nan), (3, 0.0), (beta.size - 1, -2.0), (1, np.inf)):
        bad = beta.copy()
        bad[k] = v
        refused("WaveHoltz error: cell_stiffness:", bad.ctypes.data)
        refused("WaveHoltz error: cell_stiffness:", bad.ctypes.data, precision=1)
    refused("WaveHoltz error: cell_stiffness:", beta.ctypes.data, sweep=0)
    refused("WaveHoltz error: launch:", beta.ctypes.data, launch=1)
    refused("WaveHoltz error: launch:", beta.ctypes.data, launch=1, precision=1)
    # time_ratio = 0 (from the coefficient) above the maximum
    stiff = 300.0 ** 2 * beta
    refused("WaveHoltz error: time step:", stiff.ctypes.data, ratio=0)
    rough = cd.H1Space(cd.Mesh2D.load(GOLDEN / "unstructured_square"), cd.Basis(3))
    a_rough, beta_rough = np.ones(rough.size()), np.ones(rough.mesh.n_elem())
    h = create(1.0, a_rough.ctypes.data, rough._h, 0, 1, 1, 1, None, -1, 1, 0, 0, beta_rough.ctypes.data)
    assert not h and N.last_error().startswith("WaveHoltz error: sweep:"), N.last_error()
    # the Python class reports the native message as a ValueError
    with pytest.raises(ValueError, match="WaveHoltz error: time step:"):
        cd.WaveHoltz(1.0, a, fem, stiffness="lobatto", sweep="lattice", time_ratio="coefficient", cell_stiffness=stiff)


def test_the_weight_entry_points_are_declared():
    declared = set(N.declared_symbols())
    want = {f"cuddh_hip_wave_weights_{s}_f64" for s in STAGES} | {f"cuddh_hip_wave_weights32_{s}" for s in STAGES}
    assert {s for s in declared if s.startswith("cuddh_hip_wave_weights")} == want
    assert {"cuddh_waveholtz_create_cell_stiffness", "cuddh_wave_lattice_cell_weights", "cuddh_waveholtz_coefficient_ratio"} <= declared
    for s in want:
        assert getattr(N.lib, s) is not None
