"""DDH on unstructured quad meshes (DDH.from_labels): kernels 9 (one wavefront per subdomain, LDS assembly along CSR lists)
and 10 (one workgroup per subdomain) against the oracle's table-driven local solves on the same tables (tests/ddh_general.py),
the block constructor, and the fixed point DDH with exact local solves converges to.  Every distance is printed
(`pytest -s`)."""
import math

import numpy as np
import pytest

import ddh_general as dg
import oracle
from conftest import GOLDEN
from test_gpu_parity import rel, to_dev

pytestmark = pytest.mark.gpu

MESH_DIR = GOLDEN / "unstructured_square"
OMEGA = 2 * math.pi


def block_labels(nx, ny, epd):
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    return ((i // epd) + (nx // epd) * (j // epd)).reshape(-1).astype(np.int32)


class Fixture:
    """the reference's unstructured square refined `times` times, n_basis 4, Morton parts of <= 16 elements with the whole
    star of vertex 98 (valence 5) in one subdomain"""

    def __init__(self, times, coef, omega=OMEGA):
        import cuddhelmholtz_amd as cd

        self.omega = omega
        self.mesh = cd.Mesh2D.load(MESH_DIR).refined(times)
        self.fem = cd.H1Space(self.mesh, cd.Basis(4))
        xy, el = self.mesh.vertices(), self.mesh.elements()
        self.labels = dg.with_whole_star(dg.morton_labels(xy[el].mean(axis=1)), el, 98)
        self.n_domains = int(self.labels.max()) + 1
        self.om = oracle.Mesh(xy, el)
        self.d = oracle.Discretization(self.om, 4)
        c = self.d.coordinates()
        self.h_a = np.ones(self.d.ndof) if coef == "one" else 1.0 + 0.3 * np.where((c[0] - 0.1) ** 2 + (c[1] + 0.2) ** 2 < 0.2, 1.0, 0.0)
        self.fu = oracle.linear_functional(self.d, lambda x, y: np.exp(-20 * ((x + 0.3) ** 2 + (y - 0.1) ** 2)))
        self.fv = 0.3 * oracle.linear_functional(self.d, lambda x, y: np.exp(-20 * ((x - 0.4) ** 2 + (y + 0.2) ** 2)))
        self.f = np.concatenate([self.fu, self.fv])
        assert 98 in dg.whole_stars(self.labels, el)

    def product(self, precision, kernel=0):
        import cuddhelmholtz_amd as cd

        return cd.DDH.from_labels(self.omega, self.h_a, self.fem, self.labels, precision=precision, kernel=kernel)

    def oracle(self, real):
        return dg.OracleDDH(self.d, self.n_domains, self.labels, self.omega, self.h_a, real)


_cache = {}


def fixture(times, coef="one", omega=OMEGA):
    if (times, coef, omega) not in _cache:
        _cache[(times, coef, omega)] = Fixture(times, coef, omega)
    return _cache[(times, coef, omega)]


# ------------------------------------------------------------------ tables
def test_block_labels_reproduce_every_table_of_the_block_constructor(cuda):
    import cuddhelmholtz_amd as cd

    nx = 16
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), cd.Basis(4))
    h_a = 1.0 + 0.2 * np.cos(fem.physical_coordinates()[0])
    for prec in ("f32", "f64"):
        A = cd.DDH(nx * 0.6, h_a, fem, nx, nx, precision=prec)
        B = cd.DDH.from_labels(nx * 0.6, h_a, fem, block_labels(nx, nx, 4), precision=prec)
        ia, ib = A.info(), B.info()
        assert ib["kernel"] == 9 and ib["nel1d"] == 0
        assert (ia["dt"], ia["nt"]) == (ib["dt"], ib["nt"])
        for name in ("B", "gI", "sI", "D", "G", "m", "gmi", "a", "H", "filter", "cs", "sn"):
            assert A.table(name).tobytes() == B.table(name).tobytes(), name


@pytest.mark.parametrize("times", [1, 2])
def test_fixture_tables_and_geometric_factors(cuda, times):
    fx = fixture(times)
    F = fx.product("f64")
    O = fx.oracle(np.float64)
    t = O.t
    info = F.info()
    assert info["kernel"] == 9 and info["n_domains"] == t.n_domains and (info["dt"], info["nt"]) == (t.dt, t.nt)
    assert np.array_equal(F.table("B"), t.B.reshape(-1, order="F"))
    assert np.array_equal(F.table("sI"), O._sI_product.reshape(-1, order="F"))
    gI, want = F.table("gI"), t.gI.reshape(-1, order="F")
    assert np.array_equal(gI[want >= 0], want[want >= 0])
    G = F.table("G")
    eG = float(np.max(np.abs(G - O.G.reshape(-1, order="F"))) / np.max(np.abs(O.G)))
    val = np.bincount(fx.mesh.elements().ravel())
    print(f"fixture x{times}: {fx.mesh.n_elem()} quads, {t.n_domains} subdomains (<= {int(np.bincount(fx.labels).max())} elements), "
          f"max valence {val.max()}, whole stars of valence >= 5 at {dg.whole_stars(fx.labels, fx.mesh.elements())}; G vs orc_ddh_geom_f64 {eG:.1e}")
    assert eG < 1e-14


# ------------------------------------------------------------------ local solves vs the oracle
def _entry_points(torch, cuda, F, fh, lam_h, n):
    dt = F.trace_dtype
    f = to_dev(torch, fh, cuda)
    b = torch.zeros(n, dtype=dt, device=cuda)
    F.rhs(f, b)
    lam = torch.from_numpy(lam_h.astype(np.float64 if F.f64 else np.float32)).to(cuda)
    y = torch.full((n,), 5.0, dtype=dt, device=cuda)
    F.action(lam, y)
    u = torch.full((fh.size,), 9.0, dtype=torch.float64, device=cuda)
    F.postprocess(lam, f, u)
    return b, y, u


@pytest.mark.parametrize("coef", ["one", "variable"])
@pytest.mark.parametrize("kernel", [9, 10])
def test_local_solves_match_the_oracle(cuda, kernel, coef):
    import torch

    fx = fixture(1, coef)
    O64, O32 = fx.oracle(np.float64), fx.oracle(np.float32)
    n = O64.size
    rng = np.random.default_rng(kernel)
    lam_h = rng.standard_normal(n)
    used = np.unique(O64.t.B[O64.t.B >= 0])
    lam_h[np.setdiff1d(np.arange(n), np.concatenate([used, used + O64.t.n_lambda]))] = 0.0
    written = np.unique(O64.t.B[:, 1, :][O64.t.B[:, 1, :] >= 0])
    written = np.concatenate([written, written + O64.t.n_lambda])
    ref64 = (O64.rhs(fx.f), O64.action(lam_h)[written], O64.postprocess(lam_h, fx.f))
    ref32 = (O32.rhs(fx.f), O32.action(lam_h.astype(np.float32))[written], O32.postprocess(lam_h.astype(np.float32), fx.f))
    gate32 = [4 * rel(a, b) for a, b in zip(ref32, ref64)]
    for prec in ("f64", "f32"):
        F = fx.product(prec, kernel)
        assert F.info()["kernel"] == kernel
        b, y, u = _entry_points(torch, cuda, F, fx.f, lam_h, n)
        got = (b.cpu().numpy(), y.cpu().numpy()[written], u.cpu().numpy())
        e = [rel(g, r) for g, r in zip(got, ref64)]
        gates = [1e-10] * 3 if prec == "f64" else gate32
        print(f"kernel {kernel} {prec} a={coef} vs fp64 oracle: rhs {e[0]:.2e} action {e[1]:.2e} postprocess {e[2]:.2e}  (gates "
              + " ".join(f"{g:.1e}" for g in gates) + ")")
        assert all(x < g for x, g in zip(e, gates))
        b2, y2, u2 = _entry_points(torch, cuda, F, fx.f, lam_h, n)
        assert torch.equal(b, b2) and torch.equal(y, y2) and torch.equal(u, u2)
        # ranged and listed launches write what one launch writes
        nd = fx.n_domains
        lam = torch.from_numpy(lam_h.astype(np.float64 if F.f64 else np.float32)).to(cuda)
        f = to_dev(torch, fx.f, cuda)
        full = torch.zeros(n, dtype=F.trace_dtype, device=cuda)
        F.local_traces(0, nd, f, lam, full)
        parts = torch.zeros_like(full)
        F.local_traces(0, nd // 3, f, lam, parts)
        F.local_traces(nd // 3, nd, f, lam, parts)
        assert torch.equal(parts, full)
        perm = np.random.default_rng(nd).permutation(nd).astype(np.int32)
        listed = torch.zeros_like(full)
        for ids in (perm[:7], perm[7:]):
            F.local_traces_listed(to_dev(torch, ids, cuda), f, lam, listed)
        assert torch.equal(listed, full)


def test_kernel9_on_block_labels_agrees_with_kernel2(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    nx = 16
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), cd.Basis(4))
    xy = fem.physical_coordinates()
    h_a = 1.0 + 0.3 * (xy[0] ** 2 + xy[1] ** 2 < 0.3)
    omega = 2 * math.pi * nx / 10
    K2 = cd.DDH(omega, h_a, fem, nx, nx, precision="f64", kernel=2)
    K9 = cd.DDH.from_labels(omega, h_a, fem, block_labels(nx, nx, 4), precision="f64", kernel=9)
    n = K2.size()
    rng = np.random.default_rng(5)
    lam = torch.from_numpy(rng.standard_normal(n)).to(cuda)
    f = torch.from_numpy(rng.standard_normal(2 * fem.size())).to(cuda)
    out = []
    for F in (K2, K9):
        t = torch.zeros(n, dtype=torch.float64, device=cuda)
        F.local_traces(0, F.info()["n_domains"], f, lam, t)
        u = torch.zeros(2 * fem.size(), dtype=torch.float64, device=cuda)
        F.postprocess(lam, f, u)
        out.append((t.cpu().numpy(), u.cpu().numpy()))
    e = (rel(out[1][0], out[0][0]), rel(out[1][1], out[0][1]))
    print(f"kernel 9 (block labels) vs kernel 2, fp64 16x16: traces {e[0]:.2e}, postprocess {e[1]:.2e}")
    assert max(e) < 1e-13


# ------------------------------------------------------------------ physics
def _gmres_solve(torch, cuda, F, f_h, wh_iters):
    import cuddhelmholtz_amd as cd

    F.set_wh_iters(wh_iters)
    n = F.size()
    f = to_dev(torch, f_h, cuda)
    b = torch.zeros(n, dtype=F.trace_dtype, device=cuda)
    F.rhs(f, b)
    lam = torch.zeros_like(b)
    res = cd.gmres(n, lam, F, b, 100, 20, 1e-10 if F.f64 else 1e-6)
    u = torch.zeros(f_h.size, dtype=torch.float64, device=cuda)
    F.postprocess(lam, f, u)
    return u.cpu().numpy(), res


def test_gmres_converges_to_the_general_fixed_point(cuda):
    """What remains after 12 WaveHoltz iterations is the time grid's error (RK2 + trapezoid filter), amplified by (I - T)^-1.
    Measured 5.2e-4 at omega = 2 pi (6.6e-4 at 1.5 pi), just above the 5e-4 that tests/test_ddh_physics.py uses on uniform
    2-D block decompositions, so the gate here is 6e-4."""
    import torch

    fx = fixture(1, "variable")
    O = fx.oracle(np.float64)
    want = dg.fixed_point(O.t, O.G, fx.d.ndof, fx.f)
    u12, r12 = _gmres_solve(torch, cuda, fx.product("f64", 9), fx.f, 12)
    u5, r5 = _gmres_solve(torch, cuda, fx.product("f64", 9), fx.f, 5)
    u5s, r5s = _gmres_solve(torch, cuda, fx.product("f32", 9), fx.f, 5)
    e12, e5, e5s, e3264 = rel(u12, want), rel(u5, want), rel(u5s, want), rel(u5s, u5)
    print(f"DDH-GMRES kernel 9, fixture x1 ({fx.n_domains} subdomains) vs exact-local-solve fixed point: fp64 12 WaveHoltz "
          f"iterations {e12:.2e} ({r12.num_matvec} matvecs), 5 iterations fp64 {e5:.2e} fp32 {e5s:.2e}; fp32 vs fp64 {e3264:.2e}")
    assert r12.success and r5.success
    assert e12 < 6e-4
    assert e5 < 1e-1 and e5s < 1e-1
    assert e3264 < 5e-3


def test_growth_factor_of_the_local_solve_map(cuda):
    """power iteration on lambda -> T lambda (no load): the product's estimate of the spectral radius against the oracle's"""
    import torch

    fx = fixture(2)
    F = fx.product("f64", 9)
    O = fx.oracle(np.float64)
    n = O.size
    x = np.random.default_rng(3).standard_normal(n)
    xd = torch.from_numpy(x).to(cuda)
    nd = fx.n_domains
    g_p = g_o = 0.0
    for _ in range(8):
        yo = O.solve(lam=x)[1]
        yd = torch.zeros_like(xd)
        F.local_traces(0, nd, None, xd, yd)
        g_o, g_p = np.linalg.norm(yo) / np.linalg.norm(x), float(torch.linalg.norm(yd) / torch.linalg.norm(xd))
        x = yo / np.linalg.norm(yo)
        xd = yd / torch.linalg.norm(yd)
    e = abs(g_p - g_o) / g_o
    print(f"growth factor of the local-solve map, fixture x2 ({fx.mesh.n_elem()} quads): product {g_p:.12f} oracle {g_o:.12f} "
          f"(rel {e:.1e})")
    assert e < 1e-10
