"""cd.WaveHoltz(..., stiffness="lobatto", sweep="lattice", precision="f32") on the GPU: the lattice march stored and computed in fp32.

period and action against the float64 numpy model tests/waveholtz_reference.py on the ten cases of
test_gpu_waveholtz_lattice.py::PERIOD_CASES.  The gate of a case is 4 x the error of tests/waveholtz_f32_reference.py Model32 against
that float64 model on the same case and input, computed here: the device sums with fused multiply-adds and in the lattice's order,
Model32 without them and in the matrix's, and two correct fp32 marches of 200 - 1600 steps differ from each other about as much as
each differs from float64 (Model32's errors: 0.8 - 1.5e-6).  Measured values: profiles/r26/wave_lattice_f32_tests.txt.

Bit for bit: period(None, f) = period(0, f), f = None = f = 0, two periods from one input, action(0) = 0; precision="f64" and an
omitted precision give the bits of the lattice object as it was, and report "f64".

solve: 8 x 8, rk4 / 4, GMRES(20), tol 1e-4 through cd.gmres (mgs and cgs2) and W.solve.  The models take 12 matvecs at both
precisions (tests/test_waveholtz_f32_reference.py: 11 / 12 / 13 at 2e-4 / 1e-4 / 5e-5, so 1e-4 is a factor 1.8 - 1.9 from a
change of count); the count is held to +- 1 of the f64 lattice object's in the same test, and the residual of the f32 solution
in the f64 object to 2 tol |b| (Model32: 0.56 tol; the factor 2 covers a stop one step earlier or later, the fp32 operator's own
defect adds about 1e-6).

driver: waveholtz_solve 16 4 3.2 20 100 1e-4 --integrator rk4 --coarsen 4 --sweep lattice --precision f32 against the model's 20
matvecs, +- 2; --precision f32 without --sweep lattice exits 2.
"""
import functools
import re
import subprocess

import numpy as np
import pytest

import waveholtz_f32_reference as w32
import waveholtz_reference as wr
from test_gpu_waveholtz_lattice import PERIOD_CASES, ROOT, SQUARE, dev, make, rect_case, space_of

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

GATE_FACTOR = 4.0
SOLVE_TOL = 1e-4


def make32(c, fem, scheme="rk2", coarsen=None, time_ratio=1, faces=None, **precision):
    """the lattice object at precision f32 (or what **precision says), after checking its info"""
    import cuddhelmholtz_amd as cd

    W = cd.WaveHoltz(c.omega, c.h_a, fem, integrator=scheme, coarsen=coarsen, time_ratio=time_ratio, stiffness="lobatto", faces=faces,
                     sweep="lattice", **(precision or {"precision": "f32"}))
    return W


@pytest.mark.parametrize("name", list(PERIOD_CASES))
def test_f32_period_and_action_within_four_times_the_fp32_models_error(cuda, name):
    import torch

    nx, ny, nb, box, smooth, scheme, coarsen, time_ratio, half_faces = PERIOD_CASES[name]
    c = rect_case(nx, ny, nb, box, smooth)
    fem = space_of(nx, ny, nb, box)
    faces = np.asarray(c.d.mesh.boundary_edges[::2], dtype=np.int32) if half_faces else None
    W64, M = make(c, fem, scheme, coarsen, time_ratio, "lattice", faces)  # (checks nt, dt, ratio against the model)
    W = make32(c, fem, scheme, coarsen, time_ratio, faces)
    info, info64 = W.info(), W64.info()
    assert info["precision"] == "f32" and info["sweep"] == "lattice" and info64["precision"] == "f64"
    assert info["stiffness_kernel"] == f"wave_lattice nb{nb} f32" + ("" if nb in (4, 5) else " (run-time n_basis)")
    assert {k: v for k, v in info.items() if k not in ("precision", "stiffness_kernel")} == \
           {k: v for k, v in info64.items() if k not in ("precision", "stiffness_kernel")}
    M32 = w32.Model32.of(M)
    n = W.size()
    z = np.random.default_rng(11).standard_normal(n)
    out, y, out64 = (torch.full((n,), float("nan"), dtype=torch.float64, device=cuda) for _ in range(3))
    W.period(dev(z, cuda), dev(c.f, cuda), out)
    W.action(dev(z, cuda), y)
    W64.period(dev(z, cuda), dev(c.f, cuda), out64)
    torch.cuda.synchronize()
    want, want_action = M.period(z, c.f), M.action(z)
    ref, ref_action = wr.rel(M32.period(z, c.f), want), wr.rel(M32.action(z), want_action)
    err, err_action = wr.rel(out.cpu().numpy(), want), wr.rel(y.cpu().numpy(), want_action)
    print(f"waveholtz f32 period {name}: ndof={c.d.ndof} nt={M.nt} kernel={info['stiffness_kernel']!r} vs float64 model: period {err:.3e} "
          f"(Model32 {ref:.3e}, {err / ref:.2f} x) action {err_action:.3e} (Model32 {ref_action:.3e}, {err_action / ref_action:.2f} x)")
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(y).all())
    assert 1e-8 < ref < 1e-5 and 1e-8 < ref_action < 1e-5  # an fp32 march, and a sound one
    assert err < GATE_FACTOR * ref and err_action < GATE_FACTOR * ref_action
    assert not torch.equal(out, out64)  # not the f64 object's bits: the march is in fp32


@pytest.mark.parametrize("scheme", ["rk2", "rk4"])
def test_f32_absent_arguments_and_reproducibility_bit_for_bit(cuda, scheme):
    import torch

    c = rect_case(8, 8, 4, SQUARE)
    W = make32(c, space_of(8, 8, 4, SQUARE), scheme)
    n = W.size()
    zero = torch.zeros(n, dtype=torch.float64, device=cuda)
    f, z = dev(c.f, cuda), dev(np.random.default_rng(5).standard_normal(n), cuda)
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
    want[n // 2:] *= 1.0 / c.omega
    assert torch.equal(b, want)


@pytest.mark.parametrize("scheme", ["rk2", "rk4"])
def test_default_precision_is_the_f64_lattice_object_bit_for_bit(cuda, scheme):
    import torch

    c = rect_case(8, 8, 4, SQUARE)
    fem = space_of(8, 8, 4, SQUARE)
    W0, _ = make(c, fem, scheme)  # no precision argument at all
    W1 = make32(c, fem, scheme, precision="f64")
    assert W0.info() == W1.info() and W0.info()["precision"] == "f64" and W0.info()["stiffness_kernel"] == "wave_lattice nb4"
    n = W0.size()
    f, z = dev(c.f, cuda), dev(np.random.default_rng(5).standard_normal(n), cuda)
    a, b = (torch.full((n,), float("nan"), dtype=torch.float64, device=cuda) for _ in range(2))
    W0.period(z, f, a)
    W1.period(z, f, b)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert not torch.equal(a, a.float().double())  # a double march


@functools.lru_cache(maxsize=None)
def solve_objects():
    c = rect_case(8, 8, 4, SQUARE)
    fem = space_of(8, 8, 4, SQUARE)
    return c, make32(c, fem, "rk4", 4), make(c, fem, "rk4", 4)[0]


def check_solve(cuda, what, run):
    """run(W, f, u) -> SolverOut on the f32 object and on the f64 lattice object"""
    import torch

    c, W, W64 = solve_objects()
    n = W.size()
    f = dev(c.f, cuda)
    u, u64, b, y = (torch.zeros(n, dtype=torch.float64, device=cuda) for _ in range(4))
    out, out64 = run(W, f, u), run(W64, f, u64)
    # the residual of the f32 solution in the f64 operator: z = [u; omega v]
    z = u.clone()
    z[n // 2:] *= c.omega
    W64.rhs(f, b)
    W64.action(z, y)
    res = float(torch.linalg.norm(b - y) / torch.linalg.norm(b))
    print(f"waveholtz f32 solve {what}: matvecs {out.num_matvec} (f64 lattice {out64.num_matvec}), cycles {out.num_iter}, residual of the f32 "
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
    check_solve(cuda, "WaveHoltz.solve", lambda W, f, u: W.solve(f, u, m=20, maxit=100, tol=SOLVE_TOL))


def test_waveholtz_solve_driver_f32(cuda):
    exe = ROOT / "build" / "examples" / "waveholtz_solve"
    if not exe.exists():
        pytest.fail("build/examples/waveholtz_solve missing: run __graft_entry__.build()")
    r = subprocess.run([str(exe), "16", "4", "3.2", "20", "100", "1e-4", "--integrator", "rk4", "--coarsen", "4", "--sweep", "lattice",
                        "--precision", "f32"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("waveholtz_solve")]
    assert len(lines) == 1
    print(lines[0])
    got = dict(re.findall(r"(\S+)=(\"[^\"]*\"|\S+)", lines[0]))
    c = wr.uniform_case(16, 4)
    M = c.model("rk4", 4, 1, "lobatto")
    _, info = M.gmres(c.f, 20, 100, 1e-4)
    assert info["success"] and info["num_matvec"] == 20  # recorded
    assert int(got["success"]) == 1 and abs(int(got["num_matvec"]) - info["num_matvec"]) <= 2
    assert float(got["rel_res"]) < 1e-4
    assert (got["stiffness"], got["sweep"], got["precision"], got["kernel"]) == ("lobatto", "lattice", "f32", '"wave_lattice nb4 f32"')
    assert (int(got["ndof"]), int(got["nt"]), int(got["sweeps_per_period"])) == (c.d.ndof, M.nt, 4 * M.nt)
    # the f64 line names its precision too
    r = subprocess.run([str(exe), "4", "4", "0.8", "20", "100", "1e-4", "--sweep", "lattice"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " precision=f64 " in r.stdout and 'kernel="wave_lattice nb4"' in r.stdout, r.stderr
    # the contradictions are refused
    for extra in ([], ["--sweep", "operator"], ["--stiffness", "lobatto"]):
        r = subprocess.run([str(exe), "16", "4", "--precision", "f32", *extra], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--precision f32" in r.stderr, (extra, r.stderr)
    r = subprocess.run([str(exe), "16", "4", "--sweep", "lattice", "--precision", "f16"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--precision" in r.stderr
