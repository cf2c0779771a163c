"""cd.WaveHoltz(..., sweep="lattice", launch="pair") against launch="sweep" of the same build: the same bits.

The paired march does the operations of the per-sweep march in their order, two sweeps per launch, so everything below is
torch.equal, in fp64 and in fp32: one period (RK2; RK4 with coarsen 4, with time_ratio 2 and with coarsen 3; with f = None, with
z_in = None; a 4 x 8 rectangle of 0.75 x 0.25 elements at n_basis 5; the period's step count nt is even in some cases and odd in
others, which decides where the swapped buffers end up, and each case asserts the parity it was chosen for: RK2's nt is even at
omega = 2 pi 8 / 10 on every one of these meshes, so its odd cases take omega = 2 pi 8.1 / 10, nt = 791), repeated periods on one
object (a swap that leaves state behind shows), W.solve (RK4 / 4, GMRES(20), tol 1e-6 in fp64 and 1e-4 in fp32: the same num_matvec, the same res_norm
list, the same solution), what info() reports, and the driver's --launch pair.

Two solvers are compared, so their set-up must give the same bits too.  The lumped mass is accumulated by atomic adds, and two
objects on one mesh can differ in its last bit where the elements' measures differ in theirs (a 6 x 4 mesh of [-1, 1]^2, whose
vertex coordinates round: two per-sweep objects were seen 8e-15 apart after a period, each reproducible by itself).  Every mesh
here has vertex coordinates that are exact in binary, hence equal measures and one possible sum.
"""
import functools
import math
import re
import subprocess

import numpy as np
import pytest

import waveholtz_reference as wr
from test_gpu_waveholtz_lattice import ROOT, SQUARE, dev, rect_case, space_of

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

WIDE = (-1.5, 1.5, -1.0, 1.0)  # 4 x 8 elements of 0.75 x 0.25: exact coordinates, cx = hy / hx = 1 / 3


@functools.lru_cache(maxsize=None)
def case_at(nx, ny, nb, box, tenths):
    """rect_case (omega = 2 pi max(nx, ny) / 10), or the same discretisation at omega = 2 pi tenths / 100"""
    c = rect_case(nx, ny, nb, box)
    return c if tenths is None else wr.Case(c.d, 2 * math.pi * tenths / 100)


def make(c, fem, scheme, coarsen, time_ratio, precision, launch):
    import cuddhelmholtz_amd as cd

    kw = {} if launch is None else {"launch": launch}  # None: the constructor's default
    return cd.WaveHoltz(c.omega, c.h_a, fem, integrator=scheme, coarsen=coarsen, time_ratio=time_ratio, stiffness="lobatto", sweep="lattice",
                        precision=precision, **kw)


PERIOD_CASES = {
    # id: (nx, ny, n_basis, scheme, coarsen, time_ratio, precision, with z_in, with f, nt odd[, box, omega = 2 pi this / 100])
    "8x8-rk2-f64": (8, 8, 4, "rk2", None, 1, "f64", True, True, False),
    "8x8-rk2-f32": (8, 8, 4, "rk2", None, 1, "f32", True, True, False),
    "8x8-rk2-f64-odd": (8, 8, 4, "rk2", None, 1, "f64", True, True, True, SQUARE, 81),
    "8x8-rk2-f32-odd": (8, 8, 4, "rk2", None, 1, "f32", True, True, True, SQUARE, 81),
    "8x8-rk4-f64-no-load": (8, 8, 4, "rk4", 4, 1, "f64", True, False, False),
    "8x8-rk4-f32": (8, 8, 4, "rk4", 4, 1, "f32", True, True, False),
    "8x8-rk4-ratio2-f64": (8, 8, 4, "rk4", 4, 2, "f64", True, True, False),
    "8x8-rk4-ratio2-f32-from-zero": (8, 8, 4, "rk4", 4, 2, "f32", False, True, False),
    "8x8-rk4-coarsen3-f64-from-zero": (8, 8, 4, "rk4", 3, 1, "f64", False, True, True),
    "8x8-rk4-coarsen3-f32": (8, 8, 4, "rk4", 3, 1, "f32", True, False, True),
    "4x8-nb5-rk4-f64": (4, 8, 5, "rk4", 4, 1, "f64", True, True, True, WIDE),
    "4x8-nb5-rk4-f32": (4, 8, 5, "rk4", 4, 1, "f32", True, True, True, WIDE),
    "4x8-nb5-rk2-f64": (4, 8, 5, "rk2", None, 1, "f64", True, True, False, WIDE),
}


def test_the_cases_cover_both_parities_and_both_absent_arguments():
    for scheme in ("rk2", "rk4"):
        for precision in ("f64", "f32"):
            assert {c[9] for c in PERIOD_CASES.values() if (c[3], c[6]) == (scheme, precision)} == {False, True}, (scheme, precision)
    assert any(not c[7] for c in PERIOD_CASES.values()) and any(not c[8] for c in PERIOD_CASES.values())
    assert any(c[0] != c[1] and c[2] == 5 for c in PERIOD_CASES.values())


@pytest.mark.parametrize("name", list(PERIOD_CASES))
def test_period_is_the_per_sweep_period_bit_for_bit(cuda, name):
    import torch

    nx, ny, nb, scheme, coarsen, ratio, precision, with_z, with_f, odd = PERIOD_CASES[name][:10]
    box, tenths = ((*PERIOD_CASES[name][10:], SQUARE, None) if len(PERIOD_CASES[name]) == 10 else (*PERIOD_CASES[name][10:], None))[:2]
    c = case_at(nx, ny, nb, box, tenths)
    fem = space_of(nx, ny, nb, box)
    Wp, Ws = make(c, fem, scheme, coarsen, ratio, precision, "pair"), make(c, fem, scheme, coarsen, ratio, precision, "sweep")
    ip, isw = Wp.info(), Ws.info()
    assert ip["nt"] == isw["nt"] and ip["nt"] % 2 == int(odd), ip["nt"]
    assert (ip["launch"], isw["launch"], ip["precision"], ip["sweep"]) == ("pair", "sweep", precision, "lattice")
    n = Wp.size()
    rng = np.random.default_rng(11)
    z = dev(rng.standard_normal(n), cuda) if with_z else None
    f = dev(c.f, cuda) if with_f else None
    a, b = (torch.full((n,), 7.0, dtype=torch.float64, device=cuda) for _ in range(2))
    Wp.period(z, f, a)
    Ws.period(z, f, b)
    assert bool(torch.isfinite(b).all()) and float(b.abs().max()) > 0
    assert torch.equal(a, b), f"{name}: {int((a != b).sum())} of {n} entries differ, by up to {float((a - b).abs().max()):.3e}"
    # y = x - S x goes through the same march
    if with_z:
        Wp.action(z, a)
        Ws.action(z, b)
        assert torch.equal(a, b)


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("scheme,coarsen", [("rk2", None), ("rk4", 3)], ids=["rk2", "rk4"])
def test_repeated_periods_on_one_object_are_bit_identical(cuda, scheme, coarsen, precision):
    import torch

    c = rect_case(8, 8, 4, SQUARE)
    W = make(c, space_of(8, 8, 4, SQUARE), scheme, coarsen, 1, precision, "pair")
    n = W.size()
    rng = np.random.default_rng(5)
    z, other, f = dev(rng.standard_normal(n), cuda), dev(rng.standard_normal(n), cuda), dev(c.f, cuda)
    first, again, between = (torch.empty(n, dtype=torch.float64, device=cuda) for _ in range(3))
    W.period(z, f, first)
    W.period(other, None, between)  # another period in between, homogeneous, from another state
    W.period(None, f, between)
    W.period(z, f, again)
    assert torch.equal(first, again) and float(first.abs().max()) > 0 and not torch.equal(first, between)


@pytest.mark.parametrize("precision,tol", [("f64", 1e-6), ("f32", 1e-4)])
def test_solve_takes_the_per_sweep_path(cuda, precision, tol):
    import torch

    c = rect_case(8, 8, 4, SQUARE)
    fem = space_of(8, 8, 4, SQUARE)
    f = dev(c.f, cuda)
    outs = {}
    for launch in ("pair", "sweep"):
        W = make(c, fem, "rk4", 4, 1, precision, launch)
        u = torch.zeros(W.size(), dtype=torch.float64, device=cuda)
        outs[launch] = (W.solve(f, u, m=20, maxit=100, tol=tol), u)
    (op, up), (os_, us) = outs["pair"], outs["sweep"]
    print(f"waveholtz pair solve {precision}: matvecs {op.num_matvec} / {os_.num_matvec}, res_norm {list(op.res_norm)}")
    assert os_.success and op.success and os_.num_matvec > 1
    assert op.num_matvec == os_.num_matvec and op.num_iter == os_.num_iter
    assert list(op.res_norm) == list(os_.res_norm)
    assert torch.equal(up, us) and float(us.abs().max()) > 0


def test_info_names_the_launch_and_the_kernel(cuda):
    c = rect_case(8, 8, 4, SQUARE)
    fem = space_of(8, 8, 4, SQUARE)
    default = make(c, fem, "rk4", 4, 1, "f64", None).info()
    assert (default["launch"], default["stiffness_kernel"]) == ("sweep", "wave_lattice nb4")
    assert make(c, fem, "rk4", 4, 1, "f32", None).info()["stiffness_kernel"] == "wave_lattice nb4 f32"
    for precision, kernel in (("f64", "wave_pair nb4"), ("f32", "wave_pair nb4 f32")):
        info = make(c, fem, "rk4", 4, 1, precision, "pair").info()
        assert (info["launch"], info["stiffness_kernel"], info["precision"]) == ("pair", kernel, precision)
        assert info["sweeps_per_period"] == default["sweeps_per_period"] == 4 * info["nt"]
    c3 = rect_case(6, 6, 3, SQUARE)
    assert make(c3, space_of(6, 6, 3, SQUARE), "rk2", None, 1, "f64", "pair").info()["stiffness_kernel"] == "wave_pair nb3 (run-time n_basis)"


def test_waveholtz_solve_driver_launch_pair(cuda):
    exe = ROOT / "build" / "examples" / "waveholtz_solve"
    if not exe.exists():
        pytest.fail("build/examples/waveholtz_solve missing: run __graft_entry__.build()")
    base = [str(exe), "16", "4", "3.2", "20", "100", "1e-6", "--integrator", "rk4", "--coarsen", "4", "--sweep", "lattice"]
    got = {}
    for launch, extra in (("pair", ["--launch", "pair"]), ("sweep", [])):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("waveholtz_solve")]
        assert len(lines) == 1
        print(lines[0])
        assert " precision=f64 " in lines[0] and f" launch={launch} " in lines[0]
        got[launch] = dict(re.findall(r"(\S+)=(\"[^\"]*\"|\S+)", lines[0]))
    assert got["pair"]["kernel"] == '"wave_pair nb4"' and got["sweep"]["kernel"] == '"wave_lattice nb4"'
    assert int(got["pair"]["success"]) == 1
    for key in ("num_matvec", "rel_res", "num_iter", "|u|", "nt", "sweeps_per_period"):
        assert got["pair"][key] == got["sweep"][key], key  # equal as strings
    # pair without the lattice form is refused
    r = subprocess.run([str(exe), "16", "4", "--launch", "pair"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--launch" in r.stderr
    r = subprocess.run([str(exe), "16", "4", "--sweep", "lattice", "--launch", "both"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--launch" in r.stderr
