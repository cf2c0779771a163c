"""The generated meshes of tests/irregular_meshes.py, before tests/test_gpu_irregular_meshes.py runs the plan kernels on them: the
generators themselves, the oracle on them (identities that need no reference, and its own renumbering floor), and the
preconditions of the GPU tests -- how many patches meet at a star's centre, how many colours a plan takes -- read through the
product's layout API with the inputs HelmholtzOperator hands over.  Host code: no GPU."""
import functools

import numpy as np
import pytest

import cuddhelmholtz_amd as cd
import irregular_meshes as im
import oracle
from cuddhelmholtz_amd.meshtools import refine_quads
from test_patch_layout import build_layout, space_of

FLOOR_GATE = 1e-13  # a tenth of the 1e-12 gate of the fp64 applies: a mesh the oracle cannot renumber to this is not used on the GPU


# ------------------------------------------------------------------ generators
def expected_counts(name):
    """(elements, vertices, boundary edges, boundary loops) from the generator's arguments"""
    kind, args = name.split("(")[0], [float(a) for a in name.rstrip(")").split("(")[1].split(",")]
    if kind == "star":
        k, m = int(args[0]), int(args[1])
        return k * m * m, 1 + k * m + k * m * m, 2 * k * m, 1
    if kind == "annulus":
        nt, nr = int(args[0]), int(args[1])
        return nt * nr, nt * (nr + 1), 2 * nt, 2
    if kind == "strip":
        n = int(args[0])
        return n, 2 * (n + 1), 2 * n + 2, 1
    if kind == "l_shape":
        n = int(args[0])
        return 3 * n * n // 4, (n + 1) ** 2 - (n // 2) ** 2, 4 * n, 1
    nx, ny = int(args[0]), int(args[1])
    return nx * ny, (nx + 1) * (ny + 1), 2 * (nx + ny), 1


@pytest.mark.parametrize("name", im.GPU_MESHES + ("star(32,1)", "star(5,3,0.2)"))
def test_generators_make_conforming_counter_clockwise_meshes(name):
    xy, elems = im.by_name(name)
    n_elem, n_pts, n_boundary, n_loops = expected_counts(name)
    assert elems.shape == (n_elem, 4) and xy.shape == (n_pts, 2)
    assert np.array_equal(np.unique(elems), np.arange(n_pts))  # every vertex used
    assert np.unique(xy, axis=0).shape[0] == n_pts  # and listed once
    assert np.all(im.signed_areas(xy, elems) > 0) and np.all(im.corner_turns(xy, elems) > 0)  # counter-clockwise, convex
    edges, uses = im.edge_uses(elems)
    assert set(np.unique(uses)) <= {1, 2}  # an interior edge is shared by exactly two elements
    assert np.sum(uses == 1) == n_boundary
    loops = im.boundary_loops(elems)
    assert len(loops) == n_loops and sum(map(len, loops)) == n_boundary
    if name.startswith("star"):
        k = int(name[5:].split(",")[0])
        assert np.array_equal(xy[0], (0.0, 0.0)) and np.sum(elems == 0) == k  # the valence of the centre
        assert 0 not in edges[uses == 1]
    # the product reads the same mesh: vertices, elements, boundary edges and numbering as the oracle's restatement
    pm, om = cd.Mesh2D.from_vertices(xy, elems), oracle.Mesh(xy, elems)
    assert np.array_equal(pm.vertices(), xy) and np.array_equal(pm.elements(), elems)
    assert np.array_equal(pm.boundary_edges(), np.asarray(om.boundary_edges)) and len(om.boundary_edges) == n_boundary
    I, ndof = oracle.h1_numbering(om, 3)
    fem = cd.H1Space(pm, cd.Basis(3))
    assert fem.size() == ndof and np.array_equal(fem.global_indices(), I)


def test_petals_meet_xi_axis_on_eta_axis():
    k, m = 5, 3
    xy, elems = im.star(k, m, 0.2)
    for i in range(k):
        first, nxt = elems[i * m * m:(i + 1) * m * m], elems[((i + 1) % k) * m * m:((i + 2) % k or k) * m * m]
        eta_axis = [first[b * m][0] for b in range(m)] + [first[(m - 1) * m][3]]  # s = 0: corners 0 -> 3 of the elements a = 0
        xi_axis = [nxt[a][0] for a in range(m)] + [nxt[m - 1][1]]  # t = 0: corners 0 -> 1 of the elements b = 0
        assert eta_axis == xi_axis


def test_annulus_with_one_layer_has_opposite_boundary_faces_and_strip_is_one_element_wide():
    for name in ("annulus(3,1)", "strip(5)"):
        xy, elems = im.by_name(name)
        edges = oracle.Mesh(xy, elems).edges
        sides = [[] for _ in elems]
        for e in edges:
            if e.boundary:
                sides[e.elements[0]].append(e.sides[0])
        # sides 0..3: edges (c0, c1), (c1, c2), (c3, c2), (c0, c3) -- 0 and 2 are opposite, 1 and 3 are
        assert all({0, 2} <= set(s) or {1, 3} <= set(s) for s in sides)
    assert sorted(len(s) for s in sides) == [2, 2, 2, 3, 3]  # the strip's end elements


def test_rotate_elements_keeps_the_quadrilaterals():
    xy, elems = im.rect(7, 5)
    shifts = np.random.default_rng(0).integers(0, 4, len(elems))
    turned = im.rotate_elements(elems, shifts)
    assert np.array_equal(np.sort(turned, axis=1), np.sort(elems, axis=1))
    for e in range(len(elems)):
        assert np.array_equal(turned[e], np.roll(elems[e], -shifts[e]))
    assert np.allclose(im.signed_areas(xy, turned), im.signed_areas(xy, elems), rtol=1e-15)
    assert np.array_equal(im.rotate_elements(elems, 1), np.roll(elems, -1, axis=1))


def test_product_refinement_of_a_star_matches_the_python_utility():
    xy, elems = im.star(5, 2, 0.3)
    x2, e2 = refine_quads(xy, elems, 1)
    fine = cd.Mesh2D.from_vertices(xy, elems).refined(1)
    assert fine.n_elem() == 4 * len(elems) and np.array_equal(fine.elements(), e2)
    assert np.allclose(fine.vertices(), x2, rtol=0, atol=1e-15)
    assert np.sum(fine.elements() == 0) == 5  # the centre keeps its valence


# ------------------------------------------------------------------ the oracle on these meshes, without the reference
@functools.lru_cache(maxsize=None)
def discretization(name, nb):
    return oracle.Discretization(oracle.Mesh(*im.by_name(name)), nb)


@pytest.mark.parametrize("nb", [2, 4, 7])
@pytest.mark.parametrize("name", im.GPU_MESHES)
def test_oracle_identities(name, nb):
    """S 1 = 0; 1' M 1 = area; 1' H 1 = perimeter; X' S X = area and X' S Y = 0 for the coordinate fields X, Y.  All to rounding on
    any conforming mesh of convex quadrilaterals: X and Y lie in the isoparametric space, so their physical gradients are (1, 0) and
    (0, 1) at every quadrature point, and the quadrature integrates the bilinear map's Jacobian determinant exactly."""
    xy, elems = im.by_name(name)
    d = discretization(name, nb)
    area, length = float(im.signed_areas(xy, elems).sum()), im.perimeter(xy, elems)
    one = np.ones(d.ndof)
    X, Y = d.coordinates()
    S = oracle.Stiffness(d)
    rng = np.random.default_rng(0)
    scale = np.abs(S.apply(rng.standard_normal(d.ndof))).max()  # what an entry of S x is when nothing cancels
    assert np.abs(S.apply(one)).max() <= 1e-12 * scale
    assert abs(one @ oracle.Mass(d).apply(one) - area) <= 1e-13 * area
    ofs = oracle.FaceSpaceO(d, list(d.mesh.boundary_edges))
    assert abs(oracle.FaceMass(ofs).apply(np.ones(ofs.size)).sum() - length) <= 1e-13 * length
    SX = S.apply(np.ascontiguousarray(X))
    assert abs(X @ SX - area) <= 1e-12 * area and abs(Y @ SX) <= 1e-12 * area
    assert abs(Y @ S.apply(np.ascontiguousarray(Y)) - area) <= 1e-12 * area


def match_dofs(da, db):
    """for every dof of db the dof of da at the same point, through the collocation points"""
    key = lambda d: [tuple(q) for q in np.round(d.coordinates().T * 1e7).astype(np.int64)]  # noqa: E731
    where = {k: i for i, k in enumerate(key(da))}
    assert len(where) == da.ndof == db.ndof
    match = np.array([where[k] for k in key(db)])
    assert np.array_equal(np.sort(match), np.arange(da.ndof))
    assert np.abs(da.coordinates()[:, match] - db.coordinates()).max() < 1e-13
    return match


def renumbering_floor(name, nb, seed=0):
    """relative l2 differences of the oracle's Stiffness and weighted Mass between the mesh and the same mesh with its vertices
    and elements permuted and every element's vertex list shifted: the same operator, summed in another order"""
    xy, elems = im.by_name(name)
    rng = np.random.default_rng(seed)
    vperm = rng.permutation(len(xy))  # new vertex id of old vertex v
    xy2 = np.empty_like(xy)
    xy2[vperm] = xy
    elems2 = im.rotate_elements(vperm[elems][rng.permutation(len(elems))], rng.integers(0, 4, len(elems)))
    da, db = discretization(name, nb), oracle.Discretization(oracle.Mesh(xy2, elems2), nb)
    match = match_dofs(da, db)
    x, coef = rng.standard_normal(da.ndof), 0.5 + rng.random(da.ndof)
    out = []
    for ya, yb in ((oracle.Stiffness(da).apply(x), oracle.Stiffness(db).apply(x[match])),
                   (oracle.Mass(da, coef).apply(x), oracle.Mass(db, coef[match]).apply(x[match]))):
        out.append(float(np.linalg.norm(yb - ya[match]) / np.linalg.norm(ya)))
    return out


@pytest.mark.parametrize("nb", [2, 4, 8])
@pytest.mark.parametrize("name", im.GPU_MESHES)
def test_oracle_renumbering_floor_admits_the_mesh(name, nb):
    eS, eM = renumbering_floor(name, nb)
    print(f"{name} n_basis {nb}: oracle renumbering floor, stiffness {eS:.2e}, weighted mass {eM:.2e}")
    assert eS <= FLOOR_GATE and eM <= FLOOR_GATE


# ------------------------------------------------------------------ what the GPU tests rely on, through the layout API
def slot_histogram(name, nb, pe, fused=True):
    ndof, I, xy, fI, face_elem = space_of(name, nb)
    err, L = build_layout(ndof, nb, I, xy, fI if fused else None, face_elem if fused else None, pe, fused, pe != 16)
    assert err == 0
    return np.bincount(np.diff(L["shared_off"])), L


@pytest.mark.parametrize("pe,name,patches_at_centre", [(pe, name, count) for pe, group in im.MANY_SLOT_MESHES.items() for name, count in group])
def test_patches_at_the_centre_exceed_the_four_slots_fetched_together(pe, name, patches_at_centre):
    assert patches_at_centre >= (6 if pe == 16 else 5)
    for nb in {16: (5, 6, 8), 32: (2, 5), 64: (2, 4)}[pe]:
        for fused in (True, False):
            hist, L = slot_histogram(name, nb, pe, fused)
            print(f"{name} pe {pe} n_basis {nb} {'fused' if fused else 'single'}: dofs by number of slots {dict(enumerate(hist.tolist()))}")
            slots = np.diff(L["shared_off"])
            assert slots.max() == patches_at_centre
            assert np.array_equal(L["shared_dof"][slots > 4], [I_centre(name, nb)])  # the centre vertex, and only it


def I_centre(name, nb):
    """the dof at the star's centre: vertex 0 is corner 0 of element 0"""
    return int(space_of(name, nb)[1][0, 0])


@pytest.mark.parametrize("fused", [True, False])
def test_colour_extremes(fused):
    for nb in (2, 4, 5):  # one element per lane: 32 elements per patch (fused apply), 64 (single operators; fused on request)
        for pe in (32, 64):
            ndof, I, xy, fI, face_elem = space_of("star(31,1)", nb)
            err, L = build_layout(ndof, nb, I, xy, fI if fused else None, face_elem if fused else None, pe, fused, True)
            assert err == 0 and L["ncol"] == 31 and L["n_patches"] == 1 and L["n_shared"] == 0
            for name in ("star(32,1)", "star(33,1)"):
                ndof, I, xy, fI, face_elem = space_of(name, nb)
                assert build_layout(ndof, nb, I, xy, fI if fused else None, face_elem if fused else None, pe, fused, True)[0] == 801
    # the matrix-core kernels take 16 elements per patch: at most 16 colours, so both stars get a plan there
    for name, patches in (("star(31,1)", 2), ("star(33,1)", 3)):
        ndof, I, xy, fI, face_elem = space_of(name, 6)
        err, L = build_layout(ndof, 6, I, xy, fI if fused else None, face_elem if fused else None, 16, fused, False)
        assert err == 0 and L["ncol"] == 16 and L["n_patches"] == patches and np.diff(L["shared_off"]).max() == patches
