"""cd.WaveHoltzBox(..., precision="f32") on the GPU: the three-dimensional march stored and computed in fp32.

period and action against the float64 numpy model (tests/wave_box_reference.py) on the ten cases of
test_gpu_waveholtz_box.py::PERIOD_CASES.  The gate of a case is 4 x the error of tests/waveholtz_f32_reference.py Model32 against that
float64 model on the same case and input, computed here: the project's rule for fp32 marches (test_gpu_waveholtz_f32.py).  The device
sums with fused multiply-adds and in the lattice's order, Model32 without them and in the matrix's; Model32's own errors on these
cases are 3.6e-7 to 1.6e-6 (period) and 1.8e-7 to 8.8e-7 (action), asserted to lie in (1e-8, 1e-5).  Measured ratios:
profiles/r35/wave_box_f32_tests.txt.

Bit for bit: period(None, f) = period(0, f), f = None = f = 0, two periods from one input, action(0) = 0, solution; precision="f64"
and an omitted precision give the bits, the names and the info() of the object as it was.

solve: (2, 2, 2) elements on [-1, 1]^3, n_basis 4, omega = 2 pi, the smooth coefficient, example_load, rk4 / 4, GMRES(20), tol 1e-4,
through cd.gmres (mgs and cgs2) and W.solve.  Both numpy models take 28 matvecs in 2 cycles (26 at 2e-4, 29 at 5e-5); the fp32
solution's residual in the fp64 model is 0.79 tol.  The count is held to +- 1 of the f64 object's in the same test and the residual
of the f32 solution in the f64 object to 2 tol |b|: the gates of the two-dimensional file.
"""
import functools
import math

import numpy as np
import pytest

import wave_box_reference as wb
import waveholtz_f32_reference as w32
import waveholtz_reference as wr
from test_gpu_waveholtz_box import BOX3, PERIOD_CASES, dev, make, reference

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

GATE_FACTOR = 4.0
SOLVE_TOL = 1e-4


def make32(B, omega, a, scheme="rk2", coarsen=None, time_ratio=1, **precision):
    import cuddhelmholtz_amd as cd

    Lx, Ly, Lz = B.L
    return cd.WaveHoltzBox(omega, a.reshape(Lz, Ly, Lx), shape=B.shape, box=B.box, n_basis=B.nb, integrator=scheme, coarsen=coarsen,
                           time_ratio=time_ratio, absorbing=B.absorbing, **(precision or {"precision": "f32"}))


def without(info, *keys):
    return {k: v for k, v in info.items() if k not in keys}


@pytest.mark.parametrize("name", list(PERIOD_CASES))
def test_f32_period_and_action_within_four_times_the_fp32_models_error(cuda, name):
    import torch

    shape, box, nb, omega, absorbing, (lo, hi), scheme, coarsen, time_ratio = PERIOD_CASES[name]
    B = reference(shape, box, nb, tuple(absorbing))
    a = B.smooth_coefficient(lo, hi)
    W64, M = make(B, omega, a, scheme, coarsen, time_ratio)  # (checks nt, dt, ratio against the model)
    W = make32(B, omega, a, scheme, coarsen, time_ratio)
    info, info64 = W.info(), W64.info()
    assert info["precision"] == "f32" and info64["precision"] == "f64"
    assert info["stiffness_kernel"] == f"wave_box nb{nb} f32" + ("" if nb in (4, 5) else " (run-time n_basis)") == W.kernel()
    assert without(info, "precision", "stiffness_kernel") == without(info64, "precision", "stiffness_kernel")
    assert W.lattice_shape() == B.L and W.size() == 2 * B.n
    M32 = w32.Model32.of(M)
    n = W.size()
    f = B.example_load(omega)
    z = np.random.default_rng(11).standard_normal(n)
    out, y, out64 = (torch.full((n,), float("nan"), dtype=torch.float64, device=cuda) for _ in range(3))
    W.period(dev(z, cuda), dev(f, cuda), out)
    W.action(dev(z, cuda), y)
    W64.period(dev(z, cuda), dev(f, cuda), out64)
    torch.cuda.synchronize()
    want, want_action = M.period(z, f), M.action(z)
    ref, ref_action = wr.rel(M32.period(z, f), want), wr.rel(M32.action(z), want_action)
    err, err_action = wr.rel(out.cpu().numpy(), want), wr.rel(y.cpu().numpy(), want_action)
    print(f"waveholtz box f32 period {name}: nodes={B.n} nt={M.nt} kernel={info['stiffness_kernel']!r} vs float64 model: period {err:.3e} "
          f"(Model32 {ref:.3e}, {err / ref:.2f} x) action {err_action:.3e} (Model32 {ref_action:.3e}, {err_action / ref_action:.2f} x)")
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(y).all())
    assert 1e-8 < ref < 1e-5 and 1e-8 < ref_action < 1e-5  # an fp32 march, and a sound one
    assert err < GATE_FACTOR * ref and err_action < GATE_FACTOR * ref_action
    assert not torch.equal(out, out64)  # not the f64 object's bits: the march is in fp32
    assert torch.equal(out, out.float().double())  # what leaves a period was a float


@pytest.mark.parametrize("scheme,nb", [("rk2", 4), ("rk4", 4), ("rk4", 3)])
def test_f32_absent_arguments_and_reproducibility_bit_for_bit(cuda, scheme, nb):
    import torch

    B = reference((2, 2, 2), BOX3, nb, wb.FACES)
    W = make32(B, math.pi, B.smooth_coefficient(), scheme)
    n = W.size()
    zero = torch.zeros(n, dtype=torch.float64, device=cuda)
    f, z = dev(B.example_load(math.pi), cuda), dev(np.random.default_rng(5).standard_normal(n), cuda)
    a, b = torch.empty_like(zero), torch.empty_like(zero)
    W.period(None, f, a)
    W.period(zero, f, b)
    assert torch.equal(a, b) and float(a.abs().max()) > 0
    W.rhs(f, b)
    assert torch.equal(a, b)
    W.period(z, None, a)
    W.period(z, zero, b)
    assert torch.equal(a, b) and float(a.abs().max()) > 0
    # two periods from the same input are the same bits
    W.period(z, f, a)
    W.period(z, f, b)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert torch.equal(a, a.float().double())  # what leaves a period was a float
    # action(0) = 0, and action(c, x, y) accumulates c (x - S x) in double
    W.action(zero, a)
    assert float(a.abs().max()) == 0.0
    W.action(z, a)
    y = torch.ones_like(zero)
    W.action(-0.5, z, y)
    assert wr.rel((y - 1.0).cpu().numpy(), (-0.5 * a).cpu().numpy()) < 1e-13
    W.solution(z, b)
    want = z.clone()
    want[n // 2:] *= 1.0 / math.pi
    assert torch.equal(b, want)


@pytest.mark.parametrize("scheme,nb", [("rk2", 4), ("rk4", 4), ("rk4", 5)])
def test_default_precision_is_the_f64_box_object_bit_for_bit(cuda, scheme, nb):
    import torch

    B = reference((2, 1, 2), BOX3, nb, wb.FACES)
    a = B.smooth_coefficient()
    W0, _ = make(B, math.pi, a, scheme)  # no precision argument at all
    W1 = make32(B, math.pi, a, scheme, precision="f64")
    assert W0.info() == W1.info() and W0.info()["precision"] == "f64"
    assert W0.info()["stiffness_kernel"] == f"wave_box nb{nb}" + ("" if nb == 4 else " (run-time n_basis)") == W1.kernel()
    n = W0.size()
    f, z = dev(B.example_load(math.pi), cuda), dev(np.random.default_rng(5).standard_normal(n), cuda)
    out, b = (torch.full((n,), float("nan"), dtype=torch.float64, device=cuda) for _ in range(2))
    W0.period(z, f, out)
    W1.period(z, f, b)
    assert torch.equal(out, b) and bool(torch.isfinite(out).all())
    assert not torch.equal(out, out.float().double())  # a double march


@functools.lru_cache(maxsize=None)
def solve_objects():
    B = reference((2, 2, 2), ((-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0)), 4, wb.FACES)
    a = B.smooth_coefficient()
    omega = 2 * math.pi
    return B, omega, make32(B, omega, a, "rk4", 4), make(B, omega, a, "rk4", 4)[0]


def check_solve(cuda, what, run):
    """run(W, f, u) -> SolverOut on the f32 object and on the f64 object"""
    import torch

    B, omega, W, W64 = solve_objects()
    n = W.size()
    f = dev(B.example_load(omega), cuda)
    u, u64, b, y = (torch.zeros(n, dtype=torch.float64, device=cuda) for _ in range(4))
    out, out64 = run(W, f, u), run(W64, f, u64)
    # the residual of the f32 solution in the f64 operator: z = [u; omega v]
    z = u.clone()
    z[n // 2:] *= omega
    W64.rhs(f, b)
    W64.action(z, y)
    res = float(torch.linalg.norm(b - y) / torch.linalg.norm(b))
    print(f"waveholtz box f32 solve {what}: matvecs {out.num_matvec} (f64 box {out64.num_matvec}), cycles {out.num_iter}, residual of the f32 "
          f"solution in the f64 operator {res / SOLVE_TOL:.3f} tol, solutions differ by {wr.rel(u.cpu().numpy(), u64.cpu().numpy()):.3e}")
    assert out.success and out64.success
    assert abs(out.num_matvec - out64.num_matvec) <= 1
    assert res <= 2 * SOLVE_TOL


@pytest.mark.parametrize("orth", ["mgs", "cgs2"])
def test_f32_solve_through_gmres(cuda, orth):
    import torch

    import cuddhelmholtz_amd as cd

    def run(W, f, u):
        n = W.size()
        b, z = (torch.zeros(n, dtype=torch.float64, device=cuda) for _ in range(2))
        W.rhs(f, b)
        out = cd.gmres(n, z, W, b, 20, 100, SOLVE_TOL, orth=orth)
        W.solution(z, u)
        return out

    check_solve(cuda, f"gmres orth={orth}", run)


def test_f32_solve_method(cuda):
    check_solve(cuda, "WaveHoltzBox.solve", lambda W, f, u: W.solve(f, u, m=20, maxit=100, tol=SOLVE_TOL))
