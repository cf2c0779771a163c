"""gmres(..., orth="cgs2") on the device against tests/cgs2_reference.py::gmres_cgs2_ref, and orth="mgs" through the new `_orth`
entry points against the existing ones.

Operator of most tests: HelmholtzOperator on uniform_rect(8, ...), n_basis 4 (625 nodes, vectors of 1250 doubles).  Its dense
matrix is obtained once by applying it to the unit vectors; the reference runs on that matrix.
"""
import ctypes as C
import math

import numpy as np
import pytest

import blas1_reference as br
import cgs2_reference as cr

pytestmark = pytest.mark.gpu

NX, NB, OMEGA = 8, 4, 2 * math.pi
M, MAXIT = 20, 4  # GMRES(20), three cycles


def bitwise(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


class Case:
    def __init__(self, cuda):
        import torch

        import cuddhelmholtz_amd as cd

        self.torch, self.cd, self.dev = torch, cd, cuda
        self.mesh = cd.Mesh2D.uniform_rect(NX, -1.0, 1.0, NX, -1.0, 1.0)
        self.fem = cd.H1Space(self.mesh, cd.Basis(NB))
        self.fs = cd.FaceSpace(self.fem, self.mesh.boundary_edges())
        nd = self.fem.size()
        assert nd == 625
        rng = np.random.default_rng(7)
        self.a2 = torch.from_numpy(0.5 + rng.random(nd)).to(cuda)
        self.ax = torch.from_numpy(0.5 + rng.random(self.fs.size())).to(cuda)
        self.A = cd.HelmholtzOperator(OMEGA, self.a2, self.ax, self.fem, self.fs)
        self.n = 2 * nd
        self.bh = rng.standard_normal(self.n)
        self.b = torch.from_numpy(self.bh).to(cuda)
        # the dense matrix: column j = A e_j
        eye = torch.eye(self.n, dtype=torch.float64, device=cuda)
        cols = torch.empty_like(eye)
        for j in range(self.n):
            self.A.action(eye[j], cols[j])
        self.Ad = np.ascontiguousarray(cols.cpu().numpy().T)
        # a start vector a short way from the solution: |b - A x0| = 8e-6 |b|, so that tol = 1e-6 is met in the middle of a cycle
        xs = np.linalg.solve(self.Ad, self.bh)
        dl = rng.standard_normal(self.n)
        dl *= 8e-6 * np.linalg.norm(self.bh) / np.linalg.norm(self.Ad @ dl)
        self.x0h = xs + dl
        self._ref = {}

    def reference(self, tol, T=np.float64):
        """(x, info) of gmres_cgs2_ref, computed once per (tol, type)"""
        key = (tol, T)
        if key not in self._ref:
            x0 = None if tol == 0 else self.x0h
            maxit = MAXIT if tol == 0 else 6
            self._ref[key] = cr.gmres_cgs2_ref(self.Ad, self.bh, M, maxit, tol, T, x0=x0)
        return self._ref[key]

    def start(self, tol):
        return self.torch.zeros_like(self.b) if tol == 0 else self.torch.from_numpy(self.x0h).to(self.dev)


@pytest.fixture(scope="module")
def case(cuda):
    return Case(cuda)


def out_tuple(out, x):
    return x.cpu().numpy(), np.asarray(out.res_norm, dtype=np.float64), out.num_matvec, out.num_iter, bool(out.success)


def same_run(r1, r2):
    return bitwise(r1[0], r2[0]) and bitwise(r1[1], r2[1]) and r1[2:] == r2[2:]


# ================================================================== "mgs" through the new entry points
def test_mgs_through_the_orth_entry_points_is_the_existing_path(case, monkeypatch):
    """every one of the five `_orth` entry points with orth = 0 against its counterpart: identical bits in x and res_norm, the same
    num_matvec (Python calls the existing entry points for "mgs"; here it is made to call the new ones with code 0)"""
    cd, torch, N = case.cd, case.torch, case.cd._native
    lib = N.lib
    seen = []

    def forced(name, code, head, res, h_res, h_time):
        seen.append(name + "_orth")
        return getattr(lib, name + "_orth")(*head, code, C.byref(res), h_res.ctypes.data_as(C.c_void_p), h_time.ctypes.data_as(C.c_void_p))

    nd = case.fem.size()
    h_a = np.ones(nd)
    F = cd.DDH(2 * math.pi * NX / 10, h_a, case.fem, NX, NX)
    f = torch.zeros(2 * nd, dtype=torch.float64, device=case.dev)
    cd.linear_functional(case.fem, cd.GAUSSIANS, f[:nd], param=2 * math.pi * NX / 10)
    bl = torch.zeros(F.size(), dtype=torch.float32, device=case.dev)
    F.rhs(f, bl)
    wrapped = lambda p, q: case.A.action(p, q)  # noqa: E731

    def runs():
        got = {}
        x = torch.zeros_like(case.b)
        got["helmholtz"] = out_tuple(case.A.gmres(x, case.b, M, MAXIT, 0.0), x)
        x = torch.zeros_like(case.b)
        got["f64"] = out_tuple(cd.gmres(case.n, x, case.A, case.b, M, MAXIT, 0.0), x)
        x = torch.zeros_like(case.b)
        got["callback"] = out_tuple(cd.gmres(case.n, x, wrapped, case.b, M, MAXIT, 0.0), x)
        x = torch.zeros_like(case.b)
        got["sharded"] = out_tuple(cd.gmres(case.n, x, wrapped, case.b, M, MAXIT, 0.0, reduce=lambda t: None), x)
        x = torch.zeros_like(bl)
        got["ddh"] = out_tuple(cd.gmres(F.size(), x, F, bl, 10, 20, 1e-4), x)
        return got

    old = runs()
    assert not seen
    monkeypatch.setattr(cd.api, "_gmres_entry", forced)
    new = runs()
    assert sorted(set(seen)) == sorted(["cuddh_gmres_helmholtz_orth", "cuddh_gmres_f64_orth", "cuddh_gmres_callback_orth",
                                        "cuddh_gmres_callback_sharded_orth", "cuddh_gmres_ddh_orth"])
    for name in old:
        assert same_run(old[name], new[name]), name
        assert old[name][2] > 3


# ================================================================== "cgs2" against the reference
def distance(x, r, x_ref, r_ref):
    return float(np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)), float(np.max(np.abs(r - r_ref) / np.abs(r_ref)))


def sensitivity(case):
    """float64 run against longdouble run of the reference, the longdouble results NOT rounded to float64 first (rounded, four
    residual norms that agree to half an ulp compare equal and the measured sensitivity is 0): (of x, of res_norm)"""
    xr, ir = case.reference(0.0)
    xl, il = case.reference(0.0, np.longdouble)
    rl = np.asarray(il["res_norm_unrounded"], dtype=np.longdouble)
    sx = float(np.linalg.norm(xr.astype(np.longdouble) - xl) / np.linalg.norm(xl))
    sr = float(np.max(np.abs(np.asarray(ir["res_norm"]).astype(np.longdouble) - rl) / rl))
    assert sx > 0 and sr > 0
    return sx, sr


def test_cgs2_against_the_reference(case):
    """GMRES(20), maxit 4, tol 0 under orth="cgs2": num_matvec is the reference's; x and res_norm agree with it within 10 x the
    reference's own sensitivity -- the distance between gmres_cgs2_ref in np.float64 and in np.longdouble on the same matrix
    (relative 2-norm of x, largest relative difference of res_norm; `sensitivity`), the factor 10 for the device's summation order.
    Both are printed.  On MI355X (profiles/r15/gmres_cgs2_sensitivity.txt): sensitivity 5.2e-16 (x) and 5.8e-17 (res_norm), so the
    bounds are 5.2e-15 and 5.8e-16; the device is 1.0e-15 (x) and 2.5e-16 (res_norm) from the reference."""
    xr, ir = case.reference(0.0)
    rr = np.asarray(ir["res_norm"])
    sens = sensitivity(case)
    for how in ("HelmholtzOperator.gmres", "gmres"):
        x = case.start(0.0)
        out = case.A.gmres(x, case.b, M, MAXIT, 0.0, orth="cgs2") if how == "HelmholtzOperator.gmres" else case.cd.gmres(case.n, x, case.A, case.b, M, MAXIT, 0.0, orth="cgs2")
        assert out.num_matvec == ir["num_matvec"] == 1 + (MAXIT - 1) * (M + 1)
        assert len(out.res_norm) == len(rr) and not out.success
        got = distance(x.cpu().numpy(), np.asarray(out.res_norm), xr, rr)
        print(f"{how}: num_matvec {out.num_matvec} (reference {ir['num_matvec']}); distance to the reference: x {got[0]:.3e}, res_norm {got[1]:.3e}; "
              f"the reference's sensitivity (float64 against longdouble): x {sens[0]:.3e}, res_norm {sens[1]:.3e}")
        assert got[0] <= 10 * sens[0], f"{how}: x {got[0]:.3e} from the reference, 10 x sensitivity = {10 * sens[0]:.3e}"
        assert got[1] <= 10 * sens[1], f"{how}: res_norm {got[1]:.3e} from the reference, 10 x sensitivity = {10 * sens[1]:.3e}"


def test_cgs2_converges_in_the_middle_of_a_cycle_like_the_reference(case):
    """tol = 1e-6 from a start vector 8e-6 |b| away from the solution: the inner exit test fires after a few steps of the first cycle;
    success, num_matvec and len(res_norm) are the reference's"""
    _, ir = case.reference(1e-6)
    assert ir["success"] and len(ir["res_norm"]) == 2 and 4 < ir["num_matvec"] < M  # (mid-cycle: fewer than m steps)
    x = case.start(1e-6)
    out = case.A.gmres(x, case.b, M, 6, 1e-6, orth="cgs2")
    print(f"num_matvec {out.num_matvec} (reference {ir['num_matvec']}), res_norm {list(out.res_norm)} (reference {ir['res_norm']})")
    assert bool(out.success) == ir["success"] and out.num_matvec == ir["num_matvec"] and len(out.res_norm) == len(ir["res_norm"])
    assert out.res_norm[-1] < 1e-6 * np.linalg.norm(case.bh)


# ================================================================== one step ahead against the strict path
def test_cgs2_ahead_path_equals_the_strict_path(case):
    """the operator as a handle (QueuesDeviceWorkOnly: step k + 1 is queued before the host has seen column k) and wrapped in a
    Python callable (every step waits for its column): identical bits in x and res_norm"""
    cd, torch = case.cd, case.torch
    x1, x2 = torch.zeros_like(case.b), torch.zeros_like(case.b)
    o1 = cd.gmres(case.n, x1, case.A, case.b, M, MAXIT, 0.0, orth="cgs2")
    o2 = cd.gmres(case.n, x2, lambda p, q: case.A.action(p, q), case.b, M, MAXIT, 0.0, orth="cgs2")
    assert same_run(out_tuple(o1, x1), out_tuple(o2, x2))
    # and with an early exit: the step queued ahead is discarded
    x1, x2 = case.start(1e-6), case.start(1e-6)
    o1 = cd.gmres(case.n, x1, case.A, case.b, M, 6, 1e-6, orth="cgs2")
    o2 = cd.gmres(case.n, x2, lambda p, q: case.A.action(p, q), case.b, M, 6, 1e-6, orth="cgs2")
    assert same_run(out_tuple(o1, x1), out_tuple(o2, x2)) and o1.success


# ================================================================== partitioned path with one rank
def test_cgs2_partitioned_path_with_one_rank(case):
    """reduce= with a hook that sums over one rank (nothing to do) equals the unpartitioned run bitwise: the partial sums go through
    the same summation routine either way.  The hook is called 3 times per Arnoldi step (k + 1, k + 1 and 1 scalars) plus, per
    cycle, for the residual norm and the agreed time limit, plus for |b| and the first residual; under "mgs" k + 2 times per step."""
    cd, torch = case.cd, case.torch
    op = lambda p, q: case.A.action(p, q)  # noqa: E731
    x0 = torch.zeros_like(case.b)
    plain = out_tuple(cd.gmres(case.n, x0, op, case.b, M, MAXIT, 0.0, orth="cgs2"), x0)
    calls = {"cgs2": [], "mgs": []}
    results = {}
    for orth in ("cgs2", "mgs"):
        x = torch.zeros_like(case.b)
        results[orth] = out_tuple(cd.gmres(case.n, x, op, case.b, M, MAXIT, 0.0, reduce=lambda t, o=orth: calls[o].append(t.numel()), orth=orth), x)
    assert same_run(plain, results["cgs2"])
    cycles, per_cycle = MAXIT - 1, 2
    assert len(calls["cgs2"]) == 2 + cycles * (3 * M + per_cycle)
    assert len(calls["mgs"]) == 2 + cycles * (sum(k + 2 for k in range(M)) + per_cycle)
    step = [c for k in range(M) for c in (k + 1, k + 1, 1)]
    assert calls["cgs2"] == [1, 1] + cycles * (step + [1, 1])
    assert set(calls["mgs"]) == {1}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cgs2_partitioned_path_both_precisions(cuda, dtype):
    """the same bitwise equality on a diagonal operator in either precision (1003 entries: no multiple of a 16-byte vector, so the
    basis vectors sit on a padded leading dimension)"""
    import torch

    import cuddhelmholtz_amd as cd

    n, T = 1003, getattr(torch, "float64" if dtype == "f64" else "float32")
    d = torch.linspace(1.0, 3.0, n, dtype=T, device=cuda)
    b = torch.from_numpy(np.random.default_rng(5).standard_normal(n)).to(T).to(cuda)
    op = lambda p, q: torch.mul(d, p, out=q)  # noqa: E731
    x1, x2 = torch.zeros_like(b), torch.zeros_like(b)
    o1 = cd.gmres(n, x1, op, b, 6, 4, 0.0, orth="cgs2")
    o2 = cd.gmres(n, x2, op, b, 6, 4, 0.0, reduce=lambda t: None, orth="cgs2")
    assert same_run(out_tuple(o1, x1), out_tuple(o2, x2))
    assert o1.num_matvec == 1 + 3 * 7 and o1.res_norm[-1] < 1e-3 * o1.res_norm[0]
    xr, ir = cr.gmres_cgs2_ref(lambda v: d.cpu().numpy() * v, b.cpu().numpy(), 6, 4, 0.0, br.NP[dtype])
    assert ir["num_matvec"] == o1.num_matvec
    assert np.allclose(o1.res_norm[:2], ir["res_norm"][:2], rtol=1e-3 if dtype == "f32" else 1e-9, atol=0)  # (later ones: rounding level in f32)


# ================================================================== breakdown
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cgs2_breakdown(cuda, dtype):
    """A = identity, b = e_1: h[1] == 0 exactly after the first step, the fresh basis vector is 0 / 0 and must never be used
    (as test_gpu_blas1_kernels.py::test_gmres_breakdown_through_the_callback_path for "mgs")"""
    import torch

    import cuddhelmholtz_amd as cd

    n, T = 37, br.NP[dtype]
    bh = np.zeros(n, dtype=T)
    bh[0] = 1
    b = torch.from_numpy(bh).to(cuda)
    for reduce in (None, lambda t: None):
        x = torch.zeros_like(b)
        out = cd.gmres(n, x, lambda u, v: v.copy_(u), b, 5, 10, 1e-6, reduce=reduce, orth="cgs2")
        got = x.cpu().numpy()
        assert out.success and np.all(np.isfinite(got)) and bitwise(got, bh)
        assert out.num_matvec == 3
        assert list(out.res_norm) == [1.0, 0.0]


# ================================================================== fp32 DDH
def test_cgs2_fp32_ddh_solve(cuda):
    """cd.DDH on uniform_rect(8, ...), n_basis 4 (4 subdomains), fp32 traces: rhs, then gmres(m = 10, maxit = 20, tol = 1e-4,
    orth="cgs2") succeeds, and |b - A x| recomputed through DDH.action is below 2 tol |b| (the solver's own exit test uses the same
    action; the factor 2 covers fp32 rounding of the recomputed norm).  num_matvec is printed beside the "mgs" run's, not compared."""
    import torch

    import cuddhelmholtz_amd as cd

    omega, tol = 2 * math.pi * NX / 10, 1e-4
    fem = cd.H1Space(cd.Mesh2D.uniform_rect(NX, -1.0, 1.0, NX, -1.0, 1.0), cd.Basis(NB))
    nd = fem.size()
    F = cd.DDH(omega, np.ones(nd), fem, NX, NX)
    assert F.info()["n_domains"] == 4 and F.trace_dtype == torch.float32
    f = torch.zeros(2 * nd, dtype=torch.float64, device=cuda)
    cd.linear_functional(fem, cd.GAUSSIANS, f[:nd], param=omega)
    b = torch.zeros(F.size(), dtype=torch.float32, device=cuda)
    F.rhs(f, b)
    outs = {}
    for orth in ("cgs2", "mgs"):
        x = torch.zeros_like(b)
        outs[orth] = cd.gmres(F.size(), x, F, b, 10, 20, tol, orth=orth)
        if orth == "cgs2":
            y = torch.zeros_like(b)
            F.action(x, y)
            res = float(torch.linalg.norm((b - y).double()) / torch.linalg.norm(b.double()))
    print(f"fp32 DDH 8x8: cgs2 {outs['cgs2'].num_matvec} matvecs, mgs {outs['mgs'].num_matvec}; recomputed relative residual {res:.3e}")
    assert outs["cgs2"].success
    assert res < 2 * tol
