"""The cases of tests/ddh_metric_cases.py, checked on the CPU: conditions on the meshes, the inputs and the reference that must
hold before a comparison of a device kernel with them (tests/test_gpu_ddh_metrics.py) means anything.

  * every element is valid (positive Jacobian determinant at every node) and the meshes are what the module says: the
    vertex and element numbering of the product's uniform_rect, `rect` and `shear` with one edge-vector pair for all elements
    bit for bit, `skew` with none repeated;
  * the elements are far from rectangles where they should be: the cosine between the two edge directions at an element's
    centre is 0.243 on `shear`, and reaches 0.221 (8 x 12) and 0.177 (4 x 6) on `skew`, in both signs;
  * two restatements of the reference agree: oracle.DDH (blocks of 16 / n_basis elements, tables from ddh_tables) and
    ddh_general.OracleDDH on block labels have bitwise the same tables, as tests/test_ddh_labels.py asserts on squares, and
    the same three outputs to 1e-12 (the fp64 postprocess sums its partition of unity in the threads' order: 3e-18 measured,
    everything else is bitwise equal);
  * the floors (fp32 oracle against fp64 oracle) are finite, positive and below 5e-6; measured 1.1e-7 .. 1.1e-6 in relative
    l2 and up to 3.2e-6 in max norm;
  * a metric fault cannot hide under the fp32 gate: shearing the mesh the other way, with the same coefficient, source and
    trace vectors by index, moves the fp64 outputs by 6.6e-2 .. 7.4e-1, at least 4.8e4 gates (100 is asserted);
  * a case builds in a few seconds (0.3 .. 3 s measured);
  * `tall` (hy = 2 hx, n_basis 4 only, for the element-lane kernels) meets the same conditions: valid elements, the product's
    numbering, one edge-vector pair, the two restatements, the floors; its g01 is 0 and its g00 / g11 is 4 in every node bit for
    bit where rect's is 1 / 4.  The rect inputs by index on it (swapped_rect) move the fp64 outputs by 9.8e-1 / 5.3e-1 / 1.2
    (rhs / action / postprocess), at least 3.5e5 fp32 gates of the rect case (1e4 is asserted): exchanging the x and the y
    tables of a kernel, an identity on squares, cannot hide under the gate on either.
Every figure is printed (`pytest -s`).
"""
import time

import numpy as np
import pytest

import ddh_metric_cases as mc
import oracle
from oracle.numbering import ddh_tables

SHAPE_PARAMS = [pytest.param(nb, block, id=f"nb{nb}-block{block}") for nb, block in mc.SHAPES]
CELLS = [pytest.param(f, nb, block, id=f"{f}-nb{nb}-block{block}") for nb, block in mc.SHAPES for f in mc.cells(nb, block)]
TALL = pytest.param("tall", 4, 4, id="tall-nb4-block4")  # no member of mc.FAMILIES: one shape, for the element-lane kernels
# a case is built once per session and shared with the device tests; a bound on the build keeps it that cheap.  Measured 0.3 s
# (n_basis 4) to 3 s (n_basis 8, 16 x 8 at block 8); the bound leaves a factor of ten for a slower or busier machine.
BUILD_SECONDS = 30.0
INT_TABLES = ("B", "gI", "sI", "s_dof", "s_fdof", "s_elems", "elems")
REAL_TABLES = ("D", "m", "gmi", "a", "H", "wh_filter", "cs", "sn")


@pytest.mark.parametrize("family,nb,block", CELLS + [TALL])
def test_case_builds_quickly_and_its_elements_are_valid(family, nb, block):
    # the cache is shared with every other test: the first build is timed, a cached one costs nothing
    t0 = time.perf_counter()
    c = mc.case(family, nb, block)
    seconds = time.perf_counter() - t0
    detJ = c.d.metrics(c.d.gll_x)[1]
    print(f"[{c.name}] built in {seconds:.2f} s; nt {c.O64.t.nt}, {c.O64.size} traces, {c.n_domains} subdomains; det J in "
          f"[{detJ.min():.3e}, {detJ.max():.3e}]")
    assert seconds < BUILD_SECONDS
    assert detJ.shape == (nb, nb, c.nx * c.ny) and np.isfinite(detJ).all() and detJ.min() > 0
    assert c.n_domains == (6 if block != 8 else 2) and c.n_domains % 4 != 0
    assert all(np.isfinite(r).all() and np.linalg.norm(r) > 0 for r in c.ref)
    assert np.count_nonzero(c.lam) > 0 and c.written.size > 0


@pytest.mark.parametrize("nb,block", SHAPE_PARAMS)
def test_numbering_is_the_products_uniform_rect(nb, block):
    import cuddhelmholtz_amd as cd

    nx, ny = mc.SHAPES[(nb, block)]
    for family in mc.cells(nb, block):
        xy, elems = mc.vertices(family, nx, ny)
        y0 = float(xy[0, 1]) if family in ("square", "rect") else -1.0
        base = cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, ny, y0, -y0)
        assert np.array_equal(base.elements(), elems)
        if family in ("square", "rect"):
            assert np.array_equal(base.vertices(), xy)
        mesh = cd.Mesh2D.from_vertices(xy, elems)
        assert np.array_equal(mesh.vertices(), xy) and np.array_equal(mesh.elements(), elems)


@pytest.mark.parametrize("nb,block", SHAPE_PARAMS)
def test_element_angles_and_uniformity(nb, block):
    nx, ny = mc.SHAPES[(nb, block)]

    def edge_pairs(xy, elems):
        c = xy[elems]
        return np.concatenate([c[:, 1] - c[:, 0], c[:, 2] - c[:, 3], c[:, 3] - c[:, 0], c[:, 2] - c[:, 1]], axis=1)

    for family in mc.cells(nb, block):
        xy, elems = mc.vertices(family, nx, ny)
        cs = mc.centre_cosines(xy, elems)
        pairs = edge_pairs(xy, elems)
        distinct = np.unique(pairs, axis=0).shape[0]
        print(f"[{family} {nx}x{ny}] cosine at the element centres in [{cs.min():.3f}, {cs.max():.3f}]; {distinct} distinct edge-vector sets")
        if family in ("square", "rect"):
            assert not cs.any() and distinct == 1
        elif family == "shear":
            # exact coordinates: the edge vectors, and with them the bilinear Jacobian, repeat bit for bit in every element
            assert distinct == 1
            assert cs.min() == cs.max() and cs.min() >= 0.2
            assert abs(cs[0] - mc.SHEAR / np.hypot(1.0, mc.SHEAR)) < 1e-15  # edges (hx, 0) and (SHEAR hy, hy)
        else:
            assert distinct == nx * ny
            assert cs.max() >= 0.15 and cs.min() <= -0.05  # far from a rectangle, with g01 of both signs


@pytest.mark.parametrize("family,nb,block", [p for p in CELLS if p.values[2] == 16 // p.values[1]] + [TALL])
def test_block_oracle_and_label_oracle_agree(family, nb, block):
    c = mc.case(family, nb, block)
    d = c.d
    _, Dm = oracle.basis_tables(nb, d.gll_x)
    _, detJ, _ = d.metrics(d.gll_x)
    for real, O, outs in ((np.float64, c.O64, c.ref), (np.float32, c.O32, c.out32)):
        want = ddh_tables(d.mesh, d.I, d.ndof, c.nx, c.ny, c.omega, c.h_a, d.gll_x, d.gll_w, Dm, detJ, real)
        got = O.t
        for k in ("n_domains", "n_lambda", "nt", "mx_dof", "mx_fdof", "mx_elems", "orphan_slots"):
            assert getattr(got, k) == getattr(want, k), k
        assert got.dt == want.dt
        for k in INT_TABLES:
            assert np.array_equal(getattr(got, k), getattr(want, k)), k
        for k in REAL_TABLES:
            a, b = getattr(got, k), getattr(want, k)
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
        B = oracle.DDH(d, c.nx, c.ny, c.omega, c.h_a, real)
        assert B.G.tobytes() == O.G.tobytes()
        assert np.abs(O.G[1]).max() > 0.1 * np.abs(O.G[0]).max() or family in ("square", "rect", "tall")  # g01 is there
        e = [mc.rel(a, r) for a, r in zip((B.rhs(c.fh), B.action(c.lam)[c.written], B.postprocess(c.lam, c.fh)), outs)]
        print(f"[{c.name}] oracle.DDH vs OracleDDH on block labels, {np.dtype(real).name}: tables bitwise equal; " +
              ", ".join(f"{n} {v:.1e}" for n, v in zip(mc.NAMES, e)))
        assert max(e) <= 1e-12, e


@pytest.mark.parametrize("family,nb,block", CELLS + [TALL])
def test_floors(family, nb, block):
    c = mc.case(family, nb, block)
    print(f"[{c.name}] fp32 oracle vs fp64 oracle (relative l2 / max norm): " + ", ".join(f"{n} {l2:.2e} / {mx:.2e}" for n, (l2, mx) in zip(mc.NAMES, c.floor)))
    for n, fl in zip(mc.NAMES, c.floor):
        for v in fl:
            assert np.isfinite(v) and 0 < v < 5e-6, (n, fl)


@pytest.mark.parametrize("nb,block", SHAPE_PARAMS)
def test_opposite_shear_moves_every_output_far_beyond_the_fp32_gate(nb, block):
    s, o = mc.case("shear", nb, block), mc.opposite_shear(nb, block)
    assert o.h_a is s.h_a and o.fh is s.fh and o.lam is s.lam and np.array_equal(o.written, s.written)
    assert np.array_equal(o.xy[:, 1], s.xy[:, 1]) and np.array_equal(o.xy[:, 0] + s.xy[:, 0], 2 * mc.vertices("rect", s.nx, s.ny)[0][:, 0])
    assert np.array_equal(o.O64.G[0], s.O64.G[0]) and np.array_equal(o.O64.G[2], s.O64.G[2]) and np.array_equal(o.O64.G[1], -s.O64.G[1])
    for n, a, b, (l2, _) in zip(mc.NAMES, o.ref, s.ref, s.floor):
        e, gate = mc.rel(a, b), mc.FLOOR_FACTOR * l2
        print(f"[{s.name}] {n}: g01 -> -g01 moves the fp64 reference by {e:.3e} = {e / gate:.0f} x the fp32 gate ({gate:.2e})")
        assert e >= 100 * gate, (n, e, gate)


def test_tall_is_the_rect_mesh_with_the_two_directions_exchanged():
    import cuddhelmholtz_amd as cd

    nb, block = 4, 4
    nx, ny = mc.SHAPES[(nb, block)]
    hx = 2.0 / nx
    xy, elems = mc.vertices("tall", nx, ny)
    base = cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, ny, -ny * hx, ny * hx)
    assert np.array_equal(base.elements(), elems) and np.array_equal(base.vertices(), xy)
    mesh = cd.Mesh2D.from_vertices(xy, elems)
    assert np.array_equal(mesh.vertices(), xy) and np.array_equal(mesh.elements(), elems)
    # exact coordinates: every vertex is a multiple of hx = 1/4, so every element has bit for bit the edges (hx, 0) and (0, 2 hx)
    assert np.array_equal(xy, np.round(xy / hx) * hx)
    for family, ratio in (("rect", 0.5), ("tall", 2.0)):
        v, e = mc.vertices(family, nx, ny)
        c = v[e]
        assert np.array_equal(e, elems) and not mc.centre_cosines(v, e).any()
        for a, b, want in ((1, 0, (hx, 0.0)), (2, 3, (hx, 0.0)), (3, 0, (0.0, ratio * hx)), (2, 1, (0.0, ratio * hx))):
            assert np.array_equal(c[:, a] - c[:, b], np.broadcast_to(want, (nx * ny, 2))), (family, a, b)
    # the metric the oracle marches with: G = (g00, g01, g11) per element node, node weight included
    for family, ratio in (("rect", 0.25), ("tall", 4.0)):
        k = mc.case(family, nb, block)
        for O in (k.O64, k.O32):
            g00, g01, g11 = O.G
            print(f"[{k.name}, {O.G.dtype.name}] g01 in [{g01.min():.1e}, {g01.max():.1e}]; g00 / g11 in [{(g00 / g11).min():.4f}, {(g00 / g11).max():.4f}]")
            assert g11.min() > 0 and not g01.any()
            assert np.array_equal(g00, O.G.dtype.type(ratio) * g11)  # a power of two: exact in both precisions
    r, t = mc.case("rect", nb, block), mc.case("tall", nb, block)
    assert np.array_equal(t.labels, r.labels) and np.array_equal(t.O64.t.B, r.O64.t.B) and np.array_equal(t.written, r.written)
    print(f"nt: rect {r.O64.t.nt}, tall {t.O64.t.nt}")
    assert r.O64.t.nt > t.O64.t.nt > 0


def test_exchanging_hx_and_hy_moves_every_output_far_beyond_the_fp32_gate():
    nb, block = 4, 4
    r, s = mc.case("rect", nb, block), mc.swapped_rect(nb, block)
    assert s is mc.swapped_rect(nb, block) and s.family == "tall"
    assert s.h_a is r.h_a and s.fh is r.fh and s.lam is r.lam and np.array_equal(s.written, r.written)
    assert np.array_equal(s.xy, mc.vertices("tall", r.nx, r.ny)[0]) and np.array_equal(s.elems, r.elems)
    assert np.array_equal(s.O64.G[0], 4 * s.O64.G[2]) and np.array_equal(4 * r.O64.G[0], r.O64.G[2])
    for n, fl in zip(mc.NAMES, s.floor):  # its own floors: the gate of the device's distance to its own reference
        assert all(np.isfinite(v) and 0 < v < 5e-6 for v in fl), (n, fl)
    for n, a, b, (l2, _) in zip(mc.NAMES, s.ref, r.ref, r.floor):
        e, gate = mc.rel(a, b), mc.FLOOR_FACTOR * l2
        print(f"[{r.name}] {n}: hy = hx / 2 -> hy = 2 hx moves the fp64 reference by {e:.3e} = {e / gate:.0f} x the fp32 gate ({gate:.2e})")
        assert e >= 1e4 * gate, (n, e, gate)
