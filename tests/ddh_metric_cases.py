"""DDH cases whose metric tensor is not that of a square (TEST INFRASTRUCTURE, no GPU).

Four mesh families, all with the vertex and element numbering of uniform_rect(nx, ., ., ny, ., .), so that the block kernels
(DDH(..., nx, ny, block=)) and the label-built ones (DDH.from_labels on block_labels) both take them:

  square  uniform_rect(nx, -1, 1, ny, -ny / nx, ny / nx): hx == hy, g00 == g11, g01 == 0 (what the suite had);
  rect    uniform_rect(nx, -1, 1, ny, y0, -y0) with hy = hx / 2: g00 = 1/2, g11 = 2 (times the node weight), g01 == 0;
  shear   the rect vertices with x += SHEAR * y: one metric for all elements, g01 != 0.  Every coordinate is a small
          multiple of a power of two, so every edge vector is exact and identical from element to element;
  skew    uniform_rect(nx, -1, 1, ny, -1, 1) mapped by
              x' = x + 0.08 sin(pi x) cos(pi y / 2) + 0.06 (1 - x^2) y,   y' = y + 0.07 sin(pi y) sin(pi x / 2 + 0.3):
          every element its own metric, g01 varying in sign and size; the boundary vertices in y stay on y = +-1.

A fifth, `tall`, is uniform_rect(nx, -1, 1, ny, -ny hx, ny hx) with hy = 2 hx: g00 = 2, g11 = 1/2, g01 == 0, the anisotropy of
`rect` the other way round (g00 > g11 where rect has g00 < g11).  It is no member of FAMILIES: it exists as case("tall", 4, 4) for
the element-lane kernels (tests/test_gpu_ddh_element_lane_rectangles.py), whose x and y tables are bit for bit the same on
squares.  swapped_rect is that mesh with the rect case's coefficient, sources and traces by index.

Shapes (SHAPES): the smallest with a cross point, a subdomain with three neighbours and a subdomain count (6) that is no
multiple of 4; plus 16 x 8 at block 8 (two subdomains) for kernel 11.

Inputs as in test_gpu_parity.ddh_case: coefficient alpha_disk, omega = 2 pi max(nx, ny) / 10, sources gaussians +
0.1 mass_poly, traces from default_rng(7) zeroed on the slots no subdomain reads.  The reference is
ddh_general.OracleDDH on block_labels (any block, any metric), in float64 (`ref`) and in float32; `floor` is the float32
oracle's distance to `ref` per output as (relative l2, max|a - r| / max|r|).  A case is built once (lru_cache) and nothing
in it is changed afterwards.
"""
import functools
import math

import numpy as np

import ddh_general as dg
import oracle

NAMES = ("rhs", "action", "postprocess")
FAMILIES = ("square", "rect", "shear", "skew")
SHEAR = 0.25
# (n_basis, block) -> (nx, ny)
SHAPES = {(4, 4): (8, 12), (8, 2): (4, 6), (5, 4): (8, 12), (4, 8): (16, 8)}
# the fp32 gate of tests/test_gpu_ddh_metrics.py: this many times the fp32 oracle's own distance to the fp64 oracle
FLOOR_FACTOR = 4.0
FP64_GATE = 1e-10


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / np.linalg.norm(b))


def rel_max(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - b)) / np.max(np.abs(b)))


def block_labels(nx, ny, block):
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    return ((i // block) + (nx // block) * (j // block)).reshape(-1).astype(np.int32)


def vertices(family, nx, ny, shear=SHEAR):
    """(xy, elems) of a family's mesh, numbered like uniform_rect(nx, ..., ny, ...)"""
    hx = 2.0 / nx
    if family == "square":
        y0 = -ny * hx / 2
    elif family in ("rect", "shear"):
        y0 = -ny * hx / 4
    elif family == "tall":
        y0 = -ny * hx
    elif family == "skew":
        y0 = -1.0
    else:
        raise ValueError(family)
    base = oracle.Mesh.uniform_rect(nx, -1.0, 1.0, ny, y0, -y0)
    xy = base.xy.copy()
    x, y = base.xy[:, 0], base.xy[:, 1]
    if family == "shear":
        xy[:, 0] = x + shear * y
    elif family == "skew":
        xy[:, 0] = x + 0.08 * np.sin(math.pi * x) * np.cos(math.pi * y / 2) + 0.06 * (1 - x * x) * y
        xy[:, 1] = y + 0.07 * np.sin(math.pi * y) * np.sin(math.pi * x / 2 + 0.3)
    return xy, base.elems.copy()


def centre_cosines(xy, elems):
    """per element: cosine of the angle between its two edge directions (d/dxi, d/deta of the bilinear map) at its centre"""
    c = xy[elems]  # (nel, 4, 2), counter-clockwise
    a = (c[:, 1] - c[:, 0]) + (c[:, 2] - c[:, 3])
    b = (c[:, 3] - c[:, 0]) + (c[:, 2] - c[:, 1])
    return np.einsum("ij,ij->i", a, b) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


class Case:
    """mesh, inputs and oracle outputs of one (family, n_basis, block); `like` takes the nodal coefficient, the source vector
    and the traces of another case by index (the sensitivity check), `shear` another shear factor"""

    def __init__(self, family, nb, block, shear=SHEAR, like=None):
        self.family, self.nb, self.block = family, nb, block
        self.nx, self.ny = nx, ny = SHAPES[(nb, block)]
        self.omega = 2 * math.pi * max(nx, ny) / 10
        self.xy, self.elems = vertices(family, nx, ny, shear)
        self.d = d = oracle.Discretization(oracle.Mesh(self.xy, self.elems), nb)
        self.n_domains = (nx // block) * (ny // block)
        self.labels = block_labels(nx, ny, block)
        if like is None:
            self.h_a = d.nodal(oracle.alpha_disk)
            self.fh = np.concatenate([oracle.linear_functional(d, oracle.gaussians(self.omega)), 0.1 * oracle.linear_functional(d, oracle.mass_poly)])
        else:
            self.h_a, self.fh = like.h_a, like.fh
        self.O64 = O = dg.OracleDDH(d, self.n_domains, self.labels, self.omega, self.h_a, np.float64)
        self.O32 = dg.OracleDDH(d, self.n_domains, self.labels, self.omega, self.h_a, np.float32)
        n = O.size
        B = O.t.B
        if like is None:
            lam = np.random.default_rng(7).standard_normal(n)
            used = np.unique(B[B >= 0])
            lam[np.setdiff1d(np.arange(n), np.concatenate([used, used + O.t.n_lambda]))] = 0.0
            self.lam = lam
        else:
            assert like.O64.size == n and np.array_equal(like.O64.t.B, B)
            self.lam = like.lam
        written = np.unique(B[:, 1, :][B[:, 1, :] >= 0])
        self.written = np.concatenate([written, written + O.t.n_lambda])
        self.ref = self.outputs_of(O)
        self.out32 = self.outputs_of(self.O32)
        self.floor = tuple((rel(a, r), rel_max(a, r)) for a, r in zip(self.out32, self.ref))
        for a in (self.xy, self.elems, self.h_a, self.fh, self.lam, self.written, *self.ref, *self.out32):
            a.setflags(write=False)

    def outputs_of(self, O):
        return O.rhs(self.fh), O.action(self.lam)[self.written], O.postprocess(self.lam, self.fh)

    @property
    def name(self):
        return f"{self.family} {self.nx}x{self.ny}, n_basis {self.nb}, block {self.block}"


@functools.lru_cache(maxsize=None)
def case(family, nb, block):
    return Case(family, nb, block)


@functools.lru_cache(maxsize=None)
def opposite_shear(nb, block):
    """the shear case's mesh sheared the other way, with the shear case's coefficient, sources and traces by index"""
    return Case("shear", nb, block, shear=-SHEAR, like=case("shear", nb, block))


@functools.lru_cache(maxsize=None)
def swapped_rect(nb, block):
    """the rect case's coefficient, sources and traces by index on the mesh whose hx : hy is the inverse (hy = 2 hx, not hx / 2)"""
    return Case("tall", nb, block, like=case("rect", nb, block))


def cells(nb, block):
    """the families a shape is built on: 16 x 8 at block 8 exists for kernel 11 and its refusals, on rect and shear only"""
    return ("rect", "shear") if (nb, block) == (4, 8) else FAMILIES
