"""cd.WaveHoltz(..., stiffness="lobatto", sweep="lattice") on grid meshes with missing cells (cd.Mesh2D.grid_cells): the lattice
march on csrc/kernels/wave_cells.hip / wave_cells_f32.hip.

period and action on holed meshes of 8 x 8 to 12 x 10 cells against tests/waveholtz_reference.py (Case on oracle.Mesh(xy, elems) of
the same mesh: dense K_lobatto, lumped tables, numpy march) AND against the same object built with sweep="operator", both at 1e-10
relative, the project's fp64 gate.  Cases: rk2 and rk4 / 4, a time ratio, the smooth coefficient, n_basis 3, 4, 5, 6, every boundary
edge absorbing (faces=None: the hole's walls too) and the outer boundary only (sound-hard walls).  Absent arguments and a repeated
period bit for bit.  fp32 as tests/test_gpu_waveholtz_f32.py holds it: within 4 x the distance of the float32 numpy march
(waveholtz_f32_reference.Model32) from the float64 model on the same case.

solve: the L-shape (8 x 8 less its upper right 4 x 4), rk2, GMRES(20).  The model's residual estimate is 1.860e-8 |b| after 17
matvecs and 4.940e-9 |b| after 18 (measured on the CPU; a factor 3.8 per step), so no tolerance is a factor 2 from both; 9.6e-9,
their geometric mean, is a factor 1.94 from each.  Checked here by running the model at 1.9 tol and at tol / 1.9 and asking for the
same counts (18 matvecs in one cycle); the device, whose action agrees with the model's to 1e-10, must then give that count
exactly, and res_norm to 1e-8 |b|, solution to 1e-8: the gates of tests/test_gpu_waveholtz_lattice.py.

A full grid still runs wave_lattice.hip; a full grid built through grid_cells gives the uniform_rect object's period bit for bit.
driver: waveholtz_solve --sweep lattice --void ...; with --launch pair it exits 2.
"""
import functools
import math
import re
import subprocess

import numpy as np
import pytest

import waveholtz_f32_reference as w32
import waveholtz_reference as wr
from test_gpu_waveholtz_lattice import ROOT, SQUARE, dev

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

GATE = 1e-10
GATE_FACTOR = 4.0
SOLVE_TOL = 9.6e-9


def mask(nx, ny, *holes):
    present = np.ones((ny, nx), dtype=bool)
    for i0, j0, i1, j1 in holes:
        present[j0:j1, i0:i1] = False
    return present


MESHES = {
    # name: (nx, ny, box, holes as half-open cell boxes)
    "hole-8x8": (8, 8, SQUARE, [(3, 2, 5, 5)]),
    "L-8x8": (8, 8, SQUARE, [(4, 4, 8, 8)]),
    "two-holes-12x10": (12, 10, (-1.0, 1.0, 0.0, 1.5), [(2, 2, 4, 5), (7, 6, 11, 8)]),
    "notch-10x8": (10, 8, SQUARE, [(4, 0, 6, 3), (0, 5, 1, 6)]),
    "corners-9x8": (9, 8, SQUARE, [(2, 2, 3, 3), (3, 3, 4, 4), (6, 4, 8, 5)]),
}


@functools.lru_cache(maxsize=None)
def case_and_space(name, nb, smooth=False):
    import cuddhelmholtz_amd as cd
    import oracle

    nx, ny, (ax, bx, ay, by), holes = MESHES[name]
    mesh = cd.Mesh2D.grid_cells(nx, ax, bx, ny, ay, by, mask(nx, ny, *holes))
    d = oracle.Discretization(oracle.Mesh(mesh.vertices(), mesh.elements()), nb)
    c = wr.Case(d, 2 * math.pi * max(nx, ny) / 10, wr.smooth_coefficient(d) if smooth else None)
    fem = cd.H1Space(mesh, cd.Basis(nb))
    assert fem.size() == d.ndof
    return c, fem, mesh


def outer_faces(name, mesh):
    """the boundary edges on the bounding box: the walls of the holes stay sound-hard"""
    _, _, (ax, bx, ay, by), _ = MESHES[name]
    xy, edges = mesh.vertices(), mesh.edges()
    tol = 1e-12
    keep = []
    for e in mesh.boundary_edges():
        p, q = xy[edges[e, 1]], xy[edges[e, 2]]
        on = [abs(p[0] - v) < tol and abs(q[0] - v) < tol for v in (ax, bx)] + [abs(p[1] - v) < tol and abs(q[1] - v) < tol for v in (ay, by)]
        if any(on):
            keep.append(int(e))
    assert 0 < len(keep) < len(mesh.boundary_edges())
    return np.asarray(keep, dtype=np.int32)


def make(c, fem, scheme="rk2", coarsen=None, time_ratio=1, sweep="lattice", faces=None, precision="f64"):
    import cuddhelmholtz_amd as cd

    W = cd.WaveHoltz(c.omega, c.h_a, fem, integrator=scheme, coarsen=coarsen, time_ratio=time_ratio, stiffness="lobatto", faces=faces, sweep=sweep,
                     precision=precision)
    info = W.info()
    assert info["sweep"] == sweep and info["precision"] == precision
    ratio = wr.coefficient_ratio(c.h_a) if time_ratio == "coefficient" else time_ratio
    if faces is None:
        M = c.model(scheme, info["coarsen"], ratio, "lobatto")
    else:
        m, h = wr.lumped(c.d, faces)
        M = wr.Model(c.K_lobatto, m, h, c.h_a, c.omega, c.nt(info["coarsen"], ratio), scheme)
    assert (info["nt"], info["ratio"], info["integrator"]) == (M.nt, ratio, scheme)
    assert info["sweeps_per_period"] == M.nt * (2 if scheme == "rk2" else 4) and math.isclose(info["dt"], M.dt, rel_tol=1e-15)
    return W, M


def kernel_name(nb, f32=False):
    return f"wave_cells nb{nb}" + (" f32" if f32 else "") + ("" if nb in (4, 5) else " (run-time n_basis)")


PERIOD_CASES = {
    # id: (mesh, n_basis, smooth a, scheme, coarsen, time_ratio, outer faces only)
    "hole-rk2": ("hole-8x8", 4, False, "rk2", None, 1, False),
    "hole-rk4": ("hole-8x8", 4, False, "rk4", 4, 1, False),
    "hole-sound-hard": ("hole-8x8", 4, False, "rk4", 4, 1, True),
    "L-rk2-ratio2": ("L-8x8", 4, False, "rk2", None, 2, False),
    "L-smooth-a-coefficient": ("L-8x8", 4, True, "rk4", 4, "coefficient", False),
    "two-holes-nb3": ("two-holes-12x10", 3, False, "rk2", None, 1, True),
    "notch-nb5": ("notch-10x8", 5, False, "rk4", 4, 1, False),
    "corners-nb6": ("corners-9x8", 6, False, "rk4", 4, 1, False),
    "corners-nb4-sound-hard": ("corners-9x8", 4, True, "rk2", None, 1, True),
}


@pytest.mark.parametrize("name", list(PERIOD_CASES))
def test_period_and_action_match_the_model_and_the_operator_form(cuda, name):
    import torch

    mesh_name, nb, smooth, scheme, coarsen, time_ratio, outer = PERIOD_CASES[name]
    c, fem, mesh = case_and_space(mesh_name, nb, smooth)
    faces = outer_faces(mesh_name, mesh) if outer else None
    W, M = make(c, fem, scheme, coarsen, time_ratio, "lattice", faces)
    Wo, _ = make(c, fem, scheme, coarsen, time_ratio, "operator", faces)
    assert W.info()["stiffness_kernel"] == kernel_name(nb)
    assert {k: v for k, v in W.info().items() if k not in ("sweep", "stiffness_kernel")} == \
           {k: v for k, v in Wo.info().items() if k not in ("sweep", "stiffness_kernel")}
    n = W.size()
    assert n == 2 * c.d.ndof
    z = np.random.default_rng(11).standard_normal(n)
    out, out_o, y, y_o = (torch.full((n,), float("nan"), dtype=torch.float64, device=cuda) for _ in range(4))
    W.period(dev(z, cuda), dev(c.f, cuda), out)
    Wo.period(dev(z, cuda), dev(c.f, cuda), out_o)
    W.action(dev(z, cuda), y)
    Wo.action(dev(z, cuda), y_o)
    torch.cuda.synchronize()
    want, want_action = M.period(z, c.f), M.action(z)
    err, err_action = wr.rel(out.cpu().numpy(), want), wr.rel(y.cpu().numpy(), want_action)
    err_o, err_action_o = wr.rel(out.cpu().numpy(), out_o.cpu().numpy()), wr.rel(y.cpu().numpy(), y_o.cpu().numpy())
    print(f"waveholtz cells period {name}: ndof={c.d.ndof} elems={mesh.n_elem()} nt={M.nt} kernel={W.info()['stiffness_kernel']!r} vs model: period "
          f"{err:.3e} action {err_action:.3e}; vs operator form: period {err_o:.3e} action {err_action_o:.3e}")
    assert err < GATE and err_action < GATE
    assert err_o < GATE and err_action_o < GATE
    if outer:
        assert wr.rel(want, c.model(scheme, W.info()["coarsen"], 1, "lobatto").period(z, c.f)) > 1e-3  # the walls matter


@pytest.mark.parametrize("name", ["hole-rk2", "hole-sound-hard", "two-holes-nb3", "notch-nb5", "corners-nb6"])
def test_f32_period_and_action_within_four_times_the_fp32_models_error(cuda, name):
    import torch

    mesh_name, nb, smooth, scheme, coarsen, time_ratio, outer = PERIOD_CASES[name]
    c, fem, mesh = case_and_space(mesh_name, nb, smooth)
    faces = outer_faces(mesh_name, mesh) if outer else None
    W64, M = make(c, fem, scheme, coarsen, time_ratio, "lattice", faces)
    W, _ = make(c, fem, scheme, coarsen, time_ratio, "lattice", faces, precision="f32")
    info, info64 = W.info(), W64.info()
    assert info["stiffness_kernel"] == kernel_name(nb, True)
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
    print(f"waveholtz cells f32 period {name}: ndof={c.d.ndof} nt={M.nt} kernel={info['stiffness_kernel']!r} vs float64 model: period {err:.3e} "
          f"(Model32 {ref:.3e}, {err / ref:.2f} x) action {err_action:.3e} (Model32 {ref_action:.3e}, {err_action / ref_action:.2f} x)")
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(y).all())
    assert 1e-8 < ref < 1e-5 and 1e-8 < ref_action < 1e-5  # an fp32 march, and a sound one
    assert err < GATE_FACTOR * ref and err_action < GATE_FACTOR * ref_action
    assert not torch.equal(out, out64)
    assert torch.equal(out, out.float().double())  # what leaves a period was a float


@pytest.mark.parametrize("scheme,precision", [("rk2", "f64"), ("rk4", "f64"), ("rk4", "f32")])
def test_absent_arguments_and_reproducibility_bit_for_bit(cuda, scheme, precision):
    import torch

    c, fem, _ = case_and_space("hole-8x8", 4)
    W, _ = make(c, fem, scheme, precision=precision)
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
    W.period(z, f, a)
    W.period(z, f, b)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    W.action(zero, a)
    assert float(a.abs().max()) == 0.0


@functools.lru_cache(maxsize=None)
def solve_reference():
    c, _, _ = case_and_space("L-8x8", 4)
    M = c.model("rk2", 1, 1, "lobatto")
    z, info = M.gmres(c.f, 20, 100, SOLVE_TOL)
    around = [M.gmres(c.f, 20, 100, t)[1] for t in (1.9 * SOLVE_TOL, SOLVE_TOL / 1.9)]
    return M, z, info, around


def test_solve_on_the_L_shape_follows_the_model(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    c, fem, _ = case_and_space("L-8x8", 4)
    W, _ = make(c, fem)
    n = W.size()
    b, z, u = (torch.zeros(n, dtype=torch.float64, device=cuda) for _ in range(3))
    W.rhs(dev(c.f, cuda), b)
    out = cd.gmres(n, z, W, b, 20, 100, SOLVE_TOL)
    W.solution(z, u)
    M, zm, info, around = solve_reference()
    # every comparison the model's GMRES makes against tol is a factor 1.9 away from it
    for other in around:
        assert (other["num_matvec"], other["num_iter"], other["success"]) == (info["num_matvec"], info["num_iter"], True)
    assert (info["num_matvec"], info["num_iter"]) == (18, 1)
    res, ref = np.asarray(out.res_norm), np.asarray(info["res_norm"])
    res_err = float(np.abs(res - ref).max() / ref[0]) if res.shape == ref.shape else float("inf")
    direct = M.direct(c.f)
    sol_err, distance, model_distance = wr.rel(u.cpu().numpy(), M.solution(zm)), wr.rel(u.cpu().numpy(), direct), wr.rel(M.solution(zm), direct)
    print(f"waveholtz cells solve L-8x8: matvecs {out.num_matvec} cycles {out.num_iter} (model {info['num_matvec']} / {info['num_iter']}, counts at "
          f"1.9 tol and tol / 1.9: {[o['num_matvec'] for o in around]}) res_norm vs model {res_err:.3e} of |b|, solution vs model {sol_err:.3e}, vs direct "
          f"{distance:.3e} (model {model_distance:.3e})")
    assert out.success and info["success"]
    assert (out.num_matvec, out.num_iter) == (info["num_matvec"], info["num_iter"])
    assert abs(res[0] - ref[0]) < 1e-8 * ref[0] and res_err < 1e-8
    assert sol_err < 1e-8
    assert distance < 2 * model_distance


def test_a_full_grid_keeps_the_lattice_kernels_bit_for_bit(cuda):
    import torch

    import cuddhelmholtz_amd as cd

    c = wr.uniform_case(8, 4)
    rect = cd.H1Space(cd.Mesh2D.uniform_rect(8, -1.0, 1.0, 8, -1.0, 1.0), cd.Basis(4))
    full = cd.H1Space(cd.Mesh2D.grid_cells(8, -1.0, 1.0, 8, -1.0, 1.0, np.ones((8, 8), dtype=bool)), cd.Basis(4))
    n = 2 * rect.size()
    z, f = dev(np.random.default_rng(5).standard_normal(n), cuda), dev(c.f, cuda)
    for precision, kernel in (("f64", "wave_lattice nb4"), ("f32", "wave_lattice nb4 f32")):
        outs = []
        for fem in (rect, full):
            W, _ = make(c, fem, "rk4", 4, precision=precision)
            assert W.info()["stiffness_kernel"] == kernel
            out = torch.full((n,), float("nan"), dtype=torch.float64, device=cuda)
            W.period(z, f, out)
            outs.append(out)
        assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())
    Wp = cd.WaveHoltz(c.omega, c.h_a, full, stiffness="lobatto", sweep="lattice", launch="pair")
    assert Wp.info()["stiffness_kernel"] == "wave_pair nb4"
    _, holed, _ = case_and_space("hole-8x8", 4)
    with pytest.raises(ValueError, match="WaveHoltz error: launch:"):
        cd.WaveHoltz(c.omega, np.ones(holed.size()), holed, stiffness="lobatto", sweep="lattice", launch="pair")


def test_waveholtz_solve_driver_with_voids(cuda):
    exe = ROOT / "build" / "examples" / "waveholtz_solve"
    if not exe.exists():
        pytest.fail("build/examples/waveholtz_solve missing: run __graft_entry__.build()")
    base = [str(exe), "16", "4", "3.2", "20", "100", "1e-6", "--integrator", "rk4", "--coarsen", "4", "--void", "6", "5", "10", "9", "--void", "0", "0", "2", "1"]
    got = {}
    for sweep in ("lattice", "operator"):
        r = subprocess.run(base + ["--sweep", sweep, "--stiffness", "lobatto"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("waveholtz_solve")]
        assert len(lines) == 1
        print(lines[0])
        got[sweep] = dict(re.findall(r"(\S+)=(\"[^\"]*\"|\S+)", lines[0]))
    lat, op = got["lattice"], got["operator"]
    assert lat["kernel"] == '"wave_cells nb4"' and int(lat["cells"]) == 16 * 16 - 16 - 2 == int(op["cells"])
    assert int(lat["success"]) == 1 and int(op["success"]) == 1 and float(lat["rel_res"]) < 1e-6
    assert (lat["ndof"], lat["nt"], lat["sweeps_per_period"]) == (op["ndof"], op["nt"], op["sweeps_per_period"])
    assert abs(int(lat["num_matvec"]) - int(op["num_matvec"])) <= 1 and math.isclose(float(lat["|u|"]), float(op["|u|"]), rel_tol=1e-5)
    r = subprocess.run(base + ["--sweep", "lattice", "--launch", "pair"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--launch pair" in r.stderr and not r.stdout.strip()
    r = subprocess.run([str(exe), "16", "4", "--sweep", "lattice", "--void", "3", "3", "17", "4"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--void" in r.stderr
