"""Quadrilateral meshes whose topology the fixture meshes do not have: a vertex of any valence (star), a ring with two boundary
loops (annulus), a domain one element wide (strip), a re-entrant corner (l_shape), and elements whose local vertex order is
turned (rotate_elements).  Numpy only.  Every generator returns (xy (n_pts, 2) float64, elems (n_elem, 4) int64) with
counter-clockwise quadrilaterals and every vertex listed once (ids by construction, no merging by coordinates)."""
import re

import numpy as np


def star(k, m, theta=0.0, rout=1.4):
    """k petals of m x m elements around a centre vertex of valence k.  Petal i spans the angles a0 = theta + 2 pi i / k to
    a1 = theta + 2 pi (i + 1) / k; its corners are O = (0, 0), A = (cos a0, sin a0), B = rout (cos, sin)((a0 + a1) / 2) and
    C = (cos a1, sin a1), P(s, t) is their bilinear map, and element (a, b) has the vertices P(a/m, b/m), P((a+1)/m, b/m),
    P((a+1)/m, (b+1)/m), P(a/m, (b+1)/m).  Elements petal by petal, b outer, a inner.  Petal i's eta axis (s = 0) is petal
    i+1's xi axis (t = 0)."""
    ang = theta + 2.0 * np.pi * np.arange(k) / k
    ray = np.stack([np.cos(ang), np.sin(ang)], axis=1)  # ray[i]: petal i's A and petal i-1's C
    mid = ang + np.pi / k
    tip = rout * np.stack([np.cos(mid), np.sin(mid)], axis=1)
    n_pts = 1 + k * m + k * m * m
    xy, written = np.zeros((n_pts, 2)), np.zeros(n_pts, dtype=bool)

    def vid(i, a, b):
        if a == 0 and b == 0:
            return 0
        if b == 0:  # on ray i
            return 1 + i * m + (a - 1)
        if a == 0:  # on ray i + 1
            return 1 + ((i + 1) % k) * m + (b - 1)
        return 1 + k * m + i * m * m + (b - 1) * m + (a - 1)

    elems = np.zeros((k * m * m, 4), dtype=np.int64)
    for i in range(k):
        A, B, C = ray[i], tip[i], ray[(i + 1) % k]
        for b in range(m + 1):
            for a in range(m + 1):
                s, t = a / m, b / m
                p = s * (1.0 - t) * A + s * t * B + (1.0 - s) * t * C
                v = vid(i, a, b)
                assert not written[v] or np.array_equal(xy[v], p)  # the two petals at a ray compute the same product
                xy[v], written[v] = p, True
        for b in range(m):
            for a in range(m):
                elems[i * m * m + b * m + a] = (vid(i, a, b), vid(i, a + 1, b), vid(i, a + 1, b + 1), vid(i, a, b + 1))
    return xy, elems


def annulus(nt, nr, r0=0.5, r1=1.0):
    """polygonal ring of nt x nr elements, periodic in the angle: two boundary loops (nr = 1: both on every element, on
    opposite sides).  Element (i, j) at i + nt j."""
    assert nt >= 3
    ang = 2.0 * np.pi * np.arange(nt) / nt
    r = r0 + (r1 - r0) * np.arange(nr + 1) / nr
    xy = np.stack([np.outer(r, np.cos(ang)).ravel(), np.outer(r, np.sin(ang)).ravel()], axis=1)  # vertex i + nt j
    vid = lambda i, j: (i % nt) + nt * j  # noqa: E731
    elems = np.array([(vid(i, j), vid(i, j + 1), vid(i + 1, j + 1), vid(i + 1, j)) for j in range(nr) for i in range(nt)], dtype=np.int64)
    return xy, elems


def grid(nx, ny, ax, bx, ay, by, keep=None):
    """the nx x ny rectangle grid on [ax, bx] x [ay, by] through vertices, element (i, j) in row-major order when keep(i, j);
    vertices no kept element uses are dropped"""
    x, y = ax + (bx - ax) * np.arange(nx + 1) / nx, ay + (by - ay) * np.arange(ny + 1) / ny
    xy = np.stack([np.tile(x, ny + 1), np.repeat(y, nx + 1)], axis=1)
    vid = lambda i, j: i + (nx + 1) * j  # noqa: E731
    elems = np.array([(vid(i, j), vid(i + 1, j), vid(i + 1, j + 1), vid(i, j + 1)) for j in range(ny) for i in range(nx) if keep is None or keep(i, j)],
                     dtype=np.int64)
    used = np.unique(elems)
    new_id = np.full(len(xy), -1, dtype=np.int64)
    new_id[used] = np.arange(used.size)
    return xy[used], new_id[elems]


def strip(n, hy=0.3):
    """n x 1 elements: every element has two boundary faces on opposite sides, the end ones three"""
    return grid(n, 1, -1.0, 1.0, 0.0, hy)


def l_shape(n):
    """the n x n square grid on [-1, 1]^2 without its upper right quadrant (n even)"""
    assert n % 2 == 0
    return grid(n, n, -1.0, 1.0, -1.0, 1.0, keep=lambda i, j: i < n // 2 or j < n // 2)


def rotate_elements(elems, shifts):
    """element e's vertex list shifted cyclically by shifts[e] (a scalar: every element): the same quadrilaterals, still
    counter-clockwise, with the local axes turned by shifts[e] quarter turns"""
    elems = np.asarray(elems)
    shifts = np.broadcast_to(np.asarray(shifts, dtype=np.int64), (len(elems),)) % 4
    return elems[np.arange(len(elems))[:, None], (np.arange(4)[None, :] + shifts[:, None]) % 4]


def rect(nx, ny):
    """nx x ny elements on [-1, 1]^2 through vertices (nx != ny: hx != hy, a quarter turn of the local axes swaps G00 and G11)"""
    return grid(nx, ny, -1.0, 1.0, -1.0, 1.0)


GENERATORS = {"star": star, "annulus": annulus, "strip": strip, "l_shape": l_shape, "rect": rect}

# The meshes the GPU tests run on (tests/test_gpu_irregular_meshes.py); tests/test_irregular_meshes.py admits each of them (the
# oracle's renumbering floor) and confirms, through the product's layout API, what the GPU tests rely on.
# patch size -> ((mesh, patches that must touch the centre vertex), ...): more than the four slots the border kernels fetch together
MANY_SLOT_MESHES = {
    16: (("star(8,4,0.0785,2.0)", 6), ("star(6,8,0.03,2.0)", 6)),
    32: (("star(8,7,0.4516)", 5), ("star(6,6,0.5498)", 5)),
    64: (("star(8,9,0.471)", 5), ("star(6,9,0.6283)", 5)),
}
SMALL_MESHES = ("star(3,2)", "annulus(3,1)", "annulus(7,2)", "strip(5)", "l_shape(6)")
COLOUR_MESHES = ("star(31,1)", "star(33,1)")  # 31 colours in one patch: the most a plan takes; a 32nd is refused
UNIFORM_GRIDS = ("rect(7,5)", "rect(6,6)")
GPU_MESHES = tuple(name for group in MANY_SLOT_MESHES.values() for name, _ in group) + SMALL_MESHES + COLOUR_MESHES + UNIFORM_GRIDS


def by_name(name):
    """'star(8, 4, 0.0785, 2.0)' -> star(8, 4, 0.0785, 2.0): meshes as strings, for test ids and cached lookups"""
    match = re.fullmatch(r"(\w+)\((.*)\)", name.strip())
    assert match and match.group(1) in GENERATORS, name
    args = [float(a) if any(ch in a for ch in ".e") else int(a) for a in match.group(2).split(",")]
    return GENERATORS[match.group(1)](*args)


# ---- geometry and topology in numpy, from (xy, elems) alone
def signed_areas(xy, elems):
    """shoelace area of every element (positive: counter-clockwise)"""
    p = xy[elems]  # (n_elem, 4, 2)
    q = np.roll(p, -1, axis=1)
    return 0.5 * np.sum(p[:, :, 0] * q[:, :, 1] - q[:, :, 0] * p[:, :, 1], axis=1)


def corner_turns(xy, elems):
    """(n_elem, 4) cross products of the two edges at every corner (all positive: convex and counter-clockwise)"""
    p = xy[elems]
    e_in, e_out = p - np.roll(p, 1, axis=1), np.roll(p, -1, axis=1) - p
    return e_in[:, :, 0] * e_out[:, :, 1] - e_in[:, :, 1] * e_out[:, :, 0]


def edge_uses(elems):
    """(edges (n, 2) with sorted vertex ids, how many elements use each)"""
    e = np.sort(np.stack([elems, np.roll(elems, -1, axis=1)], axis=2).reshape(-1, 2), axis=1)
    return np.unique(e, axis=0, return_counts=True)


def perimeter(xy, elems):
    edges, uses = edge_uses(elems)
    b = edges[uses == 1]
    return float(np.sum(np.hypot(*(xy[b[:, 0]] - xy[b[:, 1]]).T)))


def boundary_loops(elems):
    """the boundary edges as closed loops: a list of vertex-id lists"""
    edges, uses = edge_uses(elems)
    nxt = {}
    for a, b in edges[uses == 1]:
        nxt.setdefault(int(a), []).append(int(b))
        nxt.setdefault(int(b), []).append(int(a))
    assert all(len(v) == 2 for v in nxt.values())  # a boundary vertex lies on one loop, once
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, prev, cur = [start], None, start
        while True:
            seen.add(cur)
            a, b = nxt[cur]
            step = a if a != prev else b
            if step == start:
                break
            loop.append(step)
            prev, cur = cur, step
        loops.append(loop)
    return loops
