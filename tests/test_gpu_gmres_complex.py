"""gmres(..., arithmetic="complex") on the device: against the numpy model (tests/cgmres_reference.py) on the exact-local-solve
trace system, against the real iteration on the time-stepped DDH in fp64 and fp32, and complex_linearity_defect on both."""
import math

import numpy as np
import pytest

import cgmres_reference as cg
import lgmres_reference as lr

pytestmark = pytest.mark.gpu

M, MAXIT = 20, 100
NX, NB, BLOCK = 16, 4, 4
OMEGA = 3.2 * math.pi


class Trace:
    """trace_system(*TRACE_CASE) on the host and as a dense torch matvec, and the float64 model's run, computed once"""

    def __init__(self, dev):
        import torch

        self.Ah, self.bh = lr.trace_system(*lr.TRACE_CASE)
        self.n = len(self.bh)
        self.A, self.b = torch.from_numpy(self.Ah).to(dev), torch.from_numpy(self.bh).to(dev)
        self.op = lambda p, q: torch.mv(self.A, p, out=q)  # noqa: E731
        r = cg.TRACE_RUN
        self.x_model, self.model = cg.cgmres_ref(self.Ah, self.bh, r["m"], r["maxit"], r["tol"])


@pytest.fixture(scope="module")
def trace(cuda):
    return Trace(cuda)


class Ddh:
    """cd.DDH on uniform_rect(16, ...), n_basis 4, 4 x 4-element subdomains, omega = 3.2 pi, a = 1, and the trace right-hand side of the
    Gaussian sources; the real solve of each precision is computed once"""

    def __init__(self, dev):
        import torch

        import cuddhelmholtz_amd as cd

        self.cd, self.torch, self.dev = cd, torch, dev
        self.fem = cd.H1Space(cd.Mesh2D.uniform_rect(NX, -1.0, 1.0, NX, -1.0, 1.0), cd.Basis(NB))
        nd = self.fem.size()
        self.f = torch.zeros(2 * nd, dtype=torch.float64, device=dev)
        cd.linear_functional(self.fem, cd.GAUSSIANS, self.f[:nd], param=OMEGA)
        self._made = {}

    def get(self, precision, tol):
        """(F, b, x of the real solve, its SolverOut)"""
        if precision not in self._made:
            cd, torch = self.cd, self.torch
            F = cd.DDH(OMEGA, np.ones(self.fem.size()), self.fem, NX, NX, precision=precision, block=BLOCK)
            assert F.info()["n_domains"] == (NX // BLOCK) ** 2 and F.size() % 2 == 0
            b = torch.zeros(F.size(), dtype=F.trace_dtype, device=self.dev)
            F.rhs(self.f, b)
            x = torch.zeros_like(b)
            out = cd.gmres(F.size(), x, F, b, M, MAXIT, tol)
            self._made[precision] = (F, b, x, out)
        return self._made[precision]


@pytest.fixture(scope="module")
def ddh(cuda):
    return Ddh(cuda)


def true_residual(F, x, b):
    import torch

    y = torch.zeros_like(b)
    F.action(x, y)
    return float(torch.linalg.norm((b - y).double()) / torch.linalg.norm(b.double()))


# ================================================================== 1, 2: a callable operator against the model
def test_callable_operator_against_the_model(trace, cuda):
    """trace_system(16, 2, pi) (exact local solves: complex-linear to rounding; 1,568 complex unknowns) as a dense torch matvec in fp64,
    GMRES(20), tol 1e-6: num_matvec, the number of cycles and of residual norms are the model's; res_norm agrees with the model
    within 10 x the model's own sensitivity (float64 against longdouble on the same matrix, the longdouble run frozen in
    tests/golden/cgmres_trace_longdouble.npz; the factor 10, as in test_gpu_gmres_augment.py, for the device's summation order);
    the returned x has a true residual below tol, recomputed on the host.  The sensitivity is 1.6e-11: the last residual norms
    are 1e-6 of the first, so b - A x cancels six digits."""
    import torch

    import cuddhelmholtz_amd as cd

    ir, r = trace.model, cg.TRACE_RUN
    rr = np.asarray(ir["res_norm"])
    g = np.load(cg.golden_path())
    rl = g["res_hi"].astype(np.longdouble) + g["res_lo"]
    assert ir["success"] and int(g["num_matvec"]) == ir["num_matvec"] and len(rl) == len(rr)
    sens = float(np.max(np.abs(rr.astype(np.longdouble) - rl) / rl))
    assert sens > 0
    x = torch.zeros_like(trace.b)
    out = cd.gmres(trace.n, x, trace.op, trace.b, r["m"], r["maxit"], r["tol"], arithmetic="complex")
    got = np.asarray(out.res_norm)
    dist = float(np.max(np.abs(got - rr) / np.abs(rr))) if len(got) == len(rr) else np.inf
    res = np.linalg.norm(trace.bh - trace.Ah @ x.cpu().numpy()) / np.linalg.norm(trace.bh)
    print(f"complex: {out.num_matvec} matvecs (model {ir['num_matvec']}), {out.num_iter} cycles (model {ir['num_iter']}); res_norm {dist:.3e} from the "
          f"model, the model's sensitivity {sens:.3e}; recomputed relative residual {res:.3e}; "
          f"|x - x_model| / |x_model| = {np.linalg.norm(x.cpu().numpy() - trace.x_model) / np.linalg.norm(trace.x_model):.3e}")
    assert out.success and out.num_matvec == ir["num_matvec"]
    assert out.num_iter == ir["num_iter"] and len(got) == len(rr)
    assert dist <= 10 * sens, f"res_norm {dist:.3e} from the model, 10 x sensitivity = {10 * sens:.3e}"
    assert res < r["tol"]


def test_real_arithmetic_is_the_default_path(trace):
    """arithmetic="real" and no argument: identical res_norm, counts and x"""
    import torch

    import cuddhelmholtz_amd as cd

    x1, x2 = torch.zeros_like(trace.b), torch.zeros_like(trace.b)
    o1 = cd.gmres(trace.n, x1, trace.op, trace.b, M, 4, 1e-6)
    o2 = cd.gmres(trace.n, x2, trace.op, trace.b, M, 4, 1e-6, arithmetic="real")
    assert list(o1.res_norm) == list(o2.res_norm) and len(o1.res_norm) == 4
    assert (o1.num_matvec, o1.num_iter, o1.success) == (o2.num_matvec, o2.num_iter, o2.success)
    assert torch.equal(x1, x2)


def test_a_counting_callable_sees_num_matvec_applications(trace):
    import torch

    import cuddhelmholtz_amd as cd

    count = [0]

    def op(p, q):
        count[0] += 1
        trace.op(p, q)

    x = torch.zeros_like(trace.b)
    out = cd.gmres(trace.n, x, op, trace.b, M, 3, 0.0, arithmetic="complex")
    assert count[0] == out.num_matvec == 1 + 2 * (M + 1) and not out.success


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_breakdown_and_an_odd_half(cuda, dtype):
    """A = identity on 37 complex unknowns (an odd half: the element-wise path), b = i e_1: h[1] == 0 exactly after the first step; x = b
    exactly, three applications, residuals [1, 0] -- as on the real path"""
    import torch

    import cuddhelmholtz_amd as cd

    T = np.float64 if dtype == "f64" else np.float32
    bh = np.zeros(74, dtype=T)
    bh[37] = 1
    b = torch.from_numpy(bh).to(cuda)
    x = torch.zeros_like(b)
    out = cd.gmres(74, x, lambda u, v: v.copy_(u), b, 5, 10, 1e-6, arithmetic="complex")
    assert out.success and out.num_matvec == 3 and list(out.res_norm) == [1.0, 0.0]
    assert np.array_equal(x.cpu().numpy(), bh)


# ================================================================== 3, 4: the time-stepped DDH
def test_fp64_ddh_needs_fewer_matvecs(ddh):
    """precision="f64", GMRES(20), tol 1e-6: the complex solve succeeds; |b - F x| / |b| recomputed through F.action is below
    1.05 tol; it takes at most 0.8 x the matvecs of the real solve (numpy model of both iterations on the fp64 time-stepped
    operator: 68 against 109); x is within 1e-4 |x| of the real solve's (model: 1.6e-6)."""
    cd, torch = ddh.cd, ddh.torch
    tol = 1e-6
    F, b, x_real, o_real = ddh.get("f64", tol)
    x = torch.zeros_like(b)
    out = cd.gmres(F.size(), x, F, b, M, MAXIT, tol, arithmetic="complex")
    res, res_real = true_residual(F, x, b), true_residual(F, x_real, b)
    dx = float(torch.linalg.norm(x - x_real) / torch.linalg.norm(x_real))
    print(f"fp64 DDH 16x16: complex {out.num_matvec} matvecs, {out.num_iter} cycles, recomputed residual {res:.3e}; real {o_real.num_matvec} matvecs, "
          f"{o_real.num_iter} cycles, recomputed residual {res_real:.3e}; |x_c - x_r| / |x_r| = {dx:.3e}")
    assert o_real.success and out.success
    assert res < 1.05 * tol
    assert out.num_matvec <= 0.8 * o_real.num_matvec
    assert dx <= 1e-4


def test_fp32_ddh_needs_no_more_matvecs(ddh):
    """precision="f32", tol 1e-4: success, the recomputed true residual below 1.05 tol, no more matvecs than the real solve"""
    cd, torch = ddh.cd, ddh.torch
    tol = 1e-4
    F, b, x_real, o_real = ddh.get("f32", tol)
    assert F.trace_dtype == torch.float32
    x = torch.zeros_like(b)
    out = cd.gmres(F.size(), x, F, b, M, MAXIT, tol, arithmetic="complex")
    res = true_residual(F, x, b)
    print(f"fp32 DDH 16x16: complex {out.num_matvec} matvecs, {out.num_iter} cycles, recomputed residual {res:.3e}; real {o_real.num_matvec} matvecs, "
          f"{o_real.num_iter} cycles")
    assert o_real.success and out.success
    assert res < 1.05 * tol
    assert out.num_matvec <= o_real.num_matvec


# ================================================================== 5: the defect
def test_complex_linearity_defect(trace, ddh):
    """of the dense exact-local-solve operator: below 1e-12; of the fp64 time-stepped DDH (five WaveHoltz iterations): between
    1e-4 and 2e-2 (numpy model of that operator: 3.9e-3)"""
    import torch

    cd = ddh.cd
    exact = cd.complex_linearity_defect(trace.op, trace.n, torch.float64)
    F, *_ = ddh.get("f64", 1e-6)
    stepped = cd.complex_linearity_defect(F, F.size(), "f64", seed=1)
    print(f"complex-linearity defect: exact local solves {exact:.3e}, time-stepped fp64 DDH {stepped:.3e}")
    assert exact < 1e-12
    assert 1e-4 < stepped < 2e-2
    with pytest.raises(ValueError, match="float32"):
        cd.complex_linearity_defect(F, F.size(), "f32")
