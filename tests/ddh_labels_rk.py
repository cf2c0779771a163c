"""DDH.from_labels with per-subdomain time grids and RK4: the shared case of tests/test_ddh_labels_rk4.py (CPU) and
tests/test_gpu_ddh_labels_rk4.py (TEST INFRASTRUCTURE).

The reference's unstructured square as it is (119 quads, NOT refined), n_basis 4, omega = 2 pi, Morton
parts of <= 16 elements with the whole star of vertex 98 (valence 5) in a subdomain of its own, and a piecewise coefficient:
a = 0.4 inside the small disk, 0.5 inside the large one, 1 elsewhere, so that the `coefficient` rule gives the ratios 1, 2 and
3 and kernel 9's workgroups hold wavefronts with different step counts.  Every reference (the per-subdomain oracle, the numpy
restatement) is computed once per session and left unchanged.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import ddh_general as dg
import ddh_rk as rk
import ddh_time_grids as tg
import oracle
from conftest import GOLDEN

MESH_DIR = GOLDEN / "unstructured_square"
OMEGA = 2 * math.pi
NB = 4
COARSEN = 4
STAR_VERTEX = 98  # of valence 5; the vertex tests/test_gpu_ddh_unstructured.py keeps whole
REALS = {"f64": np.float64, "f32": np.float32}
SMALL_DISK = (0.1, -0.2, 0.05)  # centre and squared radius of a = 0.4
LARGE_DISK = (0.1, -0.2, 0.2)   # of a = 0.5


def coefficient(x, y):
    a = np.ones_like(x)
    a[(x - LARGE_DISK[0]) ** 2 + (y - LARGE_DISK[1]) ** 2 < LARGE_DISK[2]] = 0.5
    a[(x - SMALL_DISK[0]) ** 2 + (y - SMALL_DISK[1]) ** 2 < SMALL_DISK[2]] = 0.4
    return a


class LabelCase:
    """nothing in it is changed after construction"""

    def __init__(self):
        import cuddhelmholtz_amd as cd

        self.omega = OMEGA
        self.mesh = cd.Mesh2D.load(MESH_DIR)
        xy, el = self.mesh.vertices(), self.mesh.elements()
        assert el.shape == (119, 4)
        self.star_vertex = STAR_VERTEX
        assert np.bincount(el.ravel())[STAR_VERTEX] == 5
        self.labels = dg.with_whole_star(dg.morton_labels(xy[el].mean(axis=1)), el, self.star_vertex)
        assert self.star_vertex in dg.whole_stars(self.labels, el)
        self.n_domains = int(self.labels.max()) + 1
        self.d = d = oracle.Discretization(oracle.Mesh(xy, el), NB)
        c = d.coordinates()
        self.h_a = coefficient(c[0], c[1])
        self.ones = np.ones(d.ndof)
        fu = oracle.linear_functional(d, lambda x, y: np.exp(-20 * ((x + 0.3) ** 2 + (y - 0.1) ** 2)))
        fv = 0.3 * oracle.linear_functional(d, lambda x, y: np.exp(-20 * ((x - 0.4) ** 2 + (y + 0.2) ** 2)))
        self.f = np.concatenate([fu, fv])
        self.O = {name: dg.OracleDDH(d, self.n_domains, self.labels, self.omega, self.h_a, real) for name, real in REALS.items()}
        t = self.O["f64"].t
        self.nt_mesh, self.size = t.nt, self.O["f64"].size
        self.ratios = tg.coefficient_ratios(t, self.h_a)
        # what the tests rely on: three step counts, and a subdomain that leaves lanes of kernel 9's wavefront empty
        assert sorted(set(int(r) for r in self.ratios)) == [1, 2, 3], self.ratios
        assert int(np.bincount(self.labels).min()) < 16 and int(np.bincount(self.labels).max()) <= 16
        lam = np.random.default_rng(11).standard_normal(self.size)
        used = np.unique(t.B[t.B >= 0])
        lam[np.setdiff1d(np.arange(self.size), np.concatenate([used, used + t.n_lambda]))] = 0.0
        self.lam = lam
        written = np.unique(t.B[:, 1, :][t.B[:, 1, :] >= 0])
        self.written = np.concatenate([written, written + t.n_lambda])

    def fem(self):
        import cuddhelmholtz_amd as cd

        return cd.H1Space(self.mesh, cd.Basis(NB))

    def product(self, precision="f64", kernel=0, h_a=None, **kw):
        import cuddhelmholtz_amd as cd

        return cd.DDH.from_labels(self.omega, self.h_a if h_a is None else h_a, self.fem(), self.labels, precision=precision, kernel=kernel, **kw)


@functools.lru_cache(maxsize=None)
def case():
    return LabelCase()


@functools.lru_cache(maxsize=None)
def oracle_outputs(precision="f64"):
    """(rhs, action on the written slots, postprocess) of the per-subdomain RK2 oracle on the `coefficient` ratios"""
    c = case()
    P = tg.PerSubdomainOracle(c.O[precision], c.ratios)
    lam = c.lam.astype(REALS[precision])
    return P.rhs(c.f), P.action(lam)[c.written], P.postprocess(lam, c.f)


@functools.lru_cache(maxsize=None)
def restated_outputs(scheme, coarsen, with_ratios, precision="f64"):
    """the same of tests/ddh_rk.Restatement: with_ratios False is every subdomain on the base grid"""
    c = case()
    R = rk.Restatement(c.O[precision], scheme, c.ratios if with_ratios else None, coarsen)
    b, y, u = R.outputs(c.f, c.lam)
    return b, y[c.written], u
