"""The host side of the three-dimensional box solver (csrc/src/wave_box.cpp, the argument checks of
cd.WaveHoltzBox and of the C API), and tests/wave_box_reference.py, the numpy model the GPU tests rely on.  No GPU.

(a) The model: dense K, m, h by np.kron from the product's own 1-D tables.  K is symmetric and annihilates constants to
    1e-12 ||K||.  The extrusion identity ties it to what the reference pins in two dimensions: for a z-constant field,
    K3 (1 (x) p2) = (hz / 2) Wz (x) (K2 p2), m3 = (hz / 2) Wz (x) m2 and, with the four lateral faces absorbing,
    h3 = (hz / 2) Wz (x) h2, where K2, m2, h2 are waveholtz_reference.Case.K_lobatto / mh on the cross-section; all at 1e-12.
(b) cuddh_wave_box_describe against the model at 1e-12 (the project's gate for host tables) on (nx, ny, nz, n_basis) = (1,1,1,2),
    (2,1,1,3), (1,2,3,4), (2,2,1,5), (1,1,2,8), boxes with three different edge lengths, face masks none, all six and x0 alone.
(c) nt, dt and the ratio rule against waveholtz_reference.period_steps / coefficient_ratio (cuddh_waveholtz_box_time_grid).
(d) Every Python ValueError comes before any native call; every native refusal has its prefix and writes nothing.
(e) The model's GMRES fixed point against the dense direct solve of (K - w^2 M + i w H) U = f on 2 x 2 x 2 elements, n_basis 3:
    the distance is the integrator's time error, gated at twice the measured value.
"""
import ctypes as C
import math

import numpy as np
import pytest

import wave_box_reference as wb
import waveholtz_reference as wr

GATE = 1e-12
BOX3 = ((-1.0, 0.5), (0.25, 1.0), (-0.5, 1.5))  # edge lengths 1.5, 0.75, 2
DESCRIBED = [(1, 1, 1, 2), (2, 1, 1, 3), (1, 2, 3, 4), (2, 2, 1, 5), (1, 1, 2, 8)]
MASKS = [(), wb.FACES, ("x0",)]
# (e): measured, and printed by the test: distance of the model's fixed point to the direct solve (nt = 180 and 45, 32 matvecs each)
RECORDED_DISTANCE = {("rk2", 1): 6.80e-4, ("rk4", 4): 1.40e-5}


def describe(shape, box, nb, a=None, mask=63, want=("m", "h", "invm", "Hi")):
    from cuddhelmholtz_amd import _native as N

    L = [n * (nb - 1) + 1 for n in shape]
    n = L[0] * L[1] * L[2]
    stride = L[0] + L[0] % 2
    D, dims = N.WaveBox(), np.zeros(4, dtype=np.int32)
    out = {k: np.full(n, np.nan) for k in ("m", "h", "invm", "Hi")}
    dos, sod = np.full(stride * L[1] * L[2], -7, dtype=np.int32), np.full(n, -7, dtype=np.int32)
    flat = np.ascontiguousarray(box, dtype=np.float64).reshape(-1)
    err = N.lib.cuddh_wave_box_describe(*shape, flat.ctypes.data, nb, None if a is None else a.ctypes.data, mask, C.byref(D), dims.ctypes.data,
                                        *[out[k].ctypes.data for k in ("m", "h", "invm", "Hi")], dos.ctypes.data, sod.ctypes.data)
    return err, D, dims, out, dos, sod


# ------------------------------------------------------------------ (a) the model
@pytest.mark.parametrize("shape,nb", [((2, 2, 2), 3), ((1, 2, 3), 4), ((2, 1, 1), 5)])
def test_model_stiffness_is_symmetric_and_annihilates_constants(shape, nb):
    K = wb.Box(shape, BOX3, nb).K
    scale = np.linalg.norm(K, 2)
    assert np.abs(K - K.T).max() < GATE * scale
    assert np.abs(K @ np.ones(K.shape[0])).max() < GATE * scale
    assert np.all(np.linalg.eigvalsh(0.5 * (K + K.T)) > -1e-10 * scale)


@pytest.mark.parametrize("nx,ny,nz,nb", [(3, 2, 2, 4), (2, 3, 1, 3), (2, 2, 3, 5)])
def test_extrusion_identity_ties_the_model_to_the_pinned_two_dimensional_one(nx, ny, nz, nb):
    import oracle

    (ax, bx), (ay, by), (az, bz) = BOX3
    B = wb.Box((nx, ny, nz), BOX3, nb, absorbing=("x0", "x1", "y0", "y1"))
    d = oracle.Discretization(oracle.Mesh.uniform_rect(nx, ax, bx, ny, ay, by), nb)
    c = wr.Case(d, 2.0)
    # the cross-section's dofs in lattice order, by their coordinates
    xs, ys = wb.nodes_1d(ax, bx, nx, nb), wb.nodes_1d(ay, by, ny, nb)
    xy = d.coordinates()
    I = np.abs(xy[0][:, None] - xs[None, :]).argmin(axis=1)
    J = np.abs(xy[1][:, None] - ys[None, :]).argmin(axis=1)
    assert np.abs(xs[I] - xy[0]).max() < 1e-13 and np.abs(ys[J] - xy[1]).max() < 1e-13
    Lx, Ly, Lz = B.L
    dof_of = np.empty(Lx * Ly, dtype=np.int64)
    dof_of[I + Lx * J] = np.arange(d.ndof)
    assert d.ndof == Lx * Ly and np.array_equal(np.sort(dof_of), np.arange(d.ndof))
    K2 = c.K_lobatto[np.ix_(dof_of, dof_of)]
    m2, h2 = (v[dof_of] for v in c.mh)
    Wz = B.lines[2][1]
    hz = B.hs[2]
    p2 = np.random.default_rng(nb).standard_normal(Lx * Ly)
    got, want = B.K @ np.kron(np.ones(Lz), p2), hz / 2 * np.kron(Wz, K2 @ p2)
    errs = (np.abs(got - want).max() / np.abs(want).max(), np.abs(B.m - hz / 2 * np.kron(Wz, m2)).max() / B.m.max(),
            np.abs(B.h - hz / 2 * np.kron(Wz, h2)).max() / B.h.max())
    print(f"extrusion ({nx},{ny},{nz}) nb{nb}: K {errs[0]:.2e}, m {errs[1]:.2e}, h {errs[2]:.2e}")
    assert max(errs) < GATE and np.count_nonzero(B.h) == Lz * np.count_nonzero(h2)


# ------------------------------------------------------------------ (b) the host tables
@pytest.mark.parametrize("mask", MASKS, ids=["none", "all", "x0"])
@pytest.mark.parametrize("nx,ny,nz,nb", DESCRIBED)
def test_describe_is_the_model(nx, ny, nz, nb, mask):
    B = wb.Box((nx, ny, nz), BOX3, nb, absorbing=mask)
    a = B.smooth_coefficient(0.5, 2.0)
    err, D, dims, out, dos, sod = describe((nx, ny, nz), BOX3, nb, a, wb.face_mask(mask))
    assert err == 0
    Lx, Ly, Lz = B.L
    stride = Lx + Lx % 2
    assert dims.tolist() == [Lx, Ly, Lz, stride] and (D.nx, D.ny, D.nz, D.n_basis, D.stride) == (nx, ny, nz, nb, stride)
    hx, hy, hz = B.hs
    assert np.allclose([D.cx, D.cy, D.cz], [hy * hz / (2 * hx), hx * hz / (2 * hy), hx * hy / (2 * hz)], rtol=1e-15, atol=0)
    A, w = wb.tables(nb)
    assert np.array_equal(np.array(D.A[:nb * nb]).reshape(nb, nb), A) and np.array_equal(np.array(D.w[:nb]), w)
    for name, want in (("m", B.m), ("h", B.h), ("invm", 1.0 / (a * a * B.m)), ("Hi", B.h * a)):
        scale = np.abs(want).max() or 1.0
        assert np.abs(out[name] - want).max() <= GATE * scale, name
    # the corner (0, 0, 0) carries the faces through it that absorb, and nothing else
    (_, Wx), (_, Wy), (_, Wz) = B.lines
    corner = sum(c for f, c in (("x0", hy * hz / 4 * Wz[0] * Wy[0]), ("y0", hx * hz / 4 * Wz[0] * Wx[0]), ("z0", hx * hy / 4 * Wy[0] * Wx[0])) if f in mask)
    assert abs(out["h"][0] - corner) <= GATE * max(corner, 1.0) and (corner > 0) == bool({"x0", "y0", "z0"} & set(mask))
    assert np.count_nonzero(out["h"]) == np.count_nonzero(B.h)
    # the slot maps: node (I, J, K) at I + stride (J + Ly K), -1 in the padding
    g = np.arange(B.n)
    want_slot = g % Lx + stride * (g // Lx)
    assert np.array_equal(sod, want_slot) and np.array_equal(dos[want_slot], g) and np.count_nonzero(dos == -1) == (stride - Lx) * Ly * Lz
    # a == 1 where no coefficient is given
    err, *_, out1, _, _ = describe((nx, ny, nz), BOX3, nb, None, wb.face_mask(mask))
    assert err == 0 and np.abs(out1["invm"] * B.m - 1.0).max() < 1e-12 and np.abs(out1["Hi"] - B.h).max() <= GATE * (B.h.max() or 1.0)


def test_model_nodes_are_in_lattice_order():
    B = wb.Box((2, 1, 3), BOX3, 3)
    X = B.nodes
    assert X.shape == (7, 3, 5, 3)
    assert np.all(np.diff(X[0, 0, :, 0]) > 0) and np.all(np.diff(X[0, :, 0, 1]) > 0) and np.all(np.diff(X[:, 0, 0, 2]) > 0)
    assert np.allclose(X[0, 0, 0], [BOX3[0][0], BOX3[1][0], BOX3[2][0]]) and np.allclose(X[-1, -1, -1], [BOX3[0][1], BOX3[1][1], BOX3[2][1]])


# ------------------------------------------------------------------ (c) the period's grid
def time_grid(omega, shape, box, nb, a, integrator, coarsen, ratio, mask=63):
    from cuddhelmholtz_amd import _native as N

    steps, dt = np.full(2, -7, dtype=np.int32), C.c_double(-7.0)
    flat = np.ascontiguousarray(box, dtype=np.float64).reshape(-1)
    err = N.lib.cuddh_waveholtz_box_time_grid(omega, *shape, flat.ctypes.data, nb, a.ctypes.data, integrator, coarsen, ratio, mask, steps.ctypes.data,
                                              C.byref(dt))
    return err, steps.tolist(), dt.value


def test_step_counts_and_the_coefficient_ratio():
    shape, nb, omega = (3, 2, 2), 4, math.pi
    box = ((0.0, 1.5), (0.0, 1.0), (0.0, 1.0))  # h = 0.5 throughout
    n = 10 * 7 * 7
    one = np.ones(n)
    assert wr.period_steps(omega, 0.5, nb) == 640 and wr.period_steps(omega, 0.5, nb, 4) == 160
    for integrator, coarsen, ratio in ((0, 1, 1), (1, 4, 1), (1, 1, 1), (0, 1, 2), (1, 16, 3)):
        err, (nt, r), dt = time_grid(omega, shape, box, nb, one, integrator, coarsen, ratio)
        assert err == 0 and r == ratio and nt == wr.period_steps(omega, 0.5, nb, coarsen, ratio) and dt == 2.0 * math.pi / omega / nt
    # the smallest of three different mesh sizes decides
    err, (nt, _), _ = time_grid(omega, (1, 2, 3), BOX3, 3, np.ones(3 * 5 * 7), 0, 1, 1)
    assert err == 0 and nt == wr.period_steps(omega, min(1.5, 0.375, 2.0 / 3.0), 3)
    # time_ratio 0: from the coefficient
    for a_min in (0.5, 0.2, 0.3, 3.0):
        a = one.copy()
        a[17] = a_min
        err, (nt, r), _ = time_grid(omega, shape, box, nb, a, 0, 1, 0)
        assert err == 0 and r == wr.coefficient_ratio(a) and nt == wr.period_steps(omega, 0.5, nb, 1, r)
    assert wr.coefficient_ratio(np.array([0.5])) == 2 and wr.coefficient_ratio(np.array([0.2])) == 5


# ------------------------------------------------------------------ (d) refusals
def test_the_new_symbols_are_exported():
    import cuddhelmholtz_amd as cd
    from cuddhelmholtz_amd import _native as N

    assert "WaveHoltzBox" in cd.__all__ and issubclass(cd.WaveHoltzBox, cd.api._Operator)
    declared = set(N.declared_symbols())
    stages = ("rk2_a", "rk2_b", "rk4_1", "rk4_2", "rk4_3", "rk4_4")
    want = {f"cuddh_hip_wave_box_{s}_f64" for s in stages} | {f"cuddh_hip_wave_box_tile_{a}" for a in "xyz"}
    assert {s for s in declared if s.startswith("cuddh_hip_wave_box_")} == want
    assert {"cuddh_wave_box_describe", "cuddh_waveholtz_box_create", "cuddh_waveholtz_box_period", "cuddh_waveholtz_box_solution",
            "cuddh_waveholtz_box_info", "cuddh_waveholtz_box_lattice", "cuddh_waveholtz_box_time_grid"} <= declared
    for s in declared:
        if "wave_box" in s or "waveholtz_box" in s:
            assert isinstance(getattr(N.lib, s), C._CFuncPtr)
    assert (N.lib.cuddh_hip_wave_box_tile_x() >= 2 and N.lib.cuddh_hip_wave_box_tile_y() >= 1 and N.lib.cuddh_hip_wave_box_tile_z() >= 1)


GOOD = dict(omega=1.0, h_a=np.ones(8), shape=(1, 1, 1), box=((0, 1), (0, 1), (0, 1)), n_basis=2)


@pytest.mark.parametrize("kwargs,word", [
    (dict(integrator="rk3"), "integrator"),
    (dict(integrator="rk4", coarsen=17), "coarsen"),
    (dict(integrator="rk4", coarsen=True), "coarsen"),
    (dict(integrator="rk2", coarsen=2), "rk2"),
    (dict(time_ratio=0), "time_ratio"),
    (dict(time_ratio=257), "time_ratio"),
    (dict(time_ratio="mesh"), "time_ratio"),
    (dict(omega=0.0), "omega"),
    (dict(omega=float("nan")), "omega"),
    (dict(omega="1"), "omega"),
    (dict(shape=(1, 1)), "shape"),
    (dict(shape=(1, 1, 1.0)), "shape"),
    (dict(shape=3), "shape"),
    (dict(shape=(1, 0, 1)), "at least 1"),
    (dict(n_basis=1), "n_basis"),
    (dict(n_basis=9), "n_basis"),
    (dict(n_basis=4.0), "n_basis"),
    (dict(box=((0, 1), (0, 1))), "box"),
    (dict(box=((0, 1), (1, 1), (0, 1))), "box"),
    (dict(box=((0, 1), (2, 1), (0, 1))), "box"),
    (dict(box=((0, 1), (0, float("inf")), (0, 1))), "box"),
    (dict(box="unit"), "box"),
    (dict(absorbing="x0"), "absorbing"),
    (dict(absorbing=("x0", "w1")), "absorbing"),
    (dict(absorbing=("x0", "x0")), "absorbing"),
    (dict(absorbing=5), "absorbing"),
    (dict(h_a=np.ones(9)), "h_a"),
    (dict(h_a=np.ones((2, 2, 3))), "h_a"),
    (dict(h_a=np.array([1, 1, 1, 0, 1, 1, 1, 1.0])), "finite and positive"),
    (dict(h_a=np.array([1, 1, 1, -1, 1, 1, 1, 1.0])), "finite and positive"),
    (dict(h_a=np.array([1, 1, float("nan"), 1, 1, 1, 1, 1.0])), "finite and positive"),
    (dict(shape=(40000, 40000, 40000), n_basis=2), "does not fit"),
])
def test_bad_arguments_raise_before_any_native_call(monkeypatch, kwargs, word):
    import cuddhelmholtz_amd as cd

    class NoLibrary:  # any native call fails the test with another exception
        def __getattr__(self, name):
            raise AssertionError(f"{name} was called before the arguments were checked")

    monkeypatch.setattr(cd.api, "lib", NoLibrary())
    with pytest.raises(ValueError, match=word):
        cd.WaveHoltzBox(**{**GOOD, **kwargs})


def test_native_refusals_have_their_prefix_and_write_nothing():
    from cuddhelmholtz_amd import _native as N

    unit = np.array([0.0, 1.0, 0.0, 1.0, 0.0, 1.0])
    ones = np.ones(27)

    def refused(prefix, omega=1.0, shape=(1, 1, 1), box=unit, nb=3, a=ones, integrator=0, coarsen=1, ratio=1, mask=63):
        h = N.lib.cuddh_waveholtz_box_create(omega, *shape, None if box is None else box.ctypes.data, nb, None if a is None else a.ctypes.data,
                                             integrator, coarsen, ratio, mask)
        assert not h and N.last_error().startswith(prefix), (prefix, N.last_error())
        steps, dt = np.full(2, -7, dtype=np.int32), C.c_double(-7.0)
        err = N.lib.cuddh_waveholtz_box_time_grid(omega, *shape, None if box is None else box.ctypes.data, nb, None if a is None else a.ctypes.data,
                                                  integrator, coarsen, ratio, mask, steps.ctypes.data, C.byref(dt))
        assert err != 0 and N.last_error().startswith(prefix) and steps.tolist() == [-7, -7] and dt.value == -7.0

    for shape in ((0, 1, 1), (1, -1, 1), (1, 1, 0)):
        refused("WaveHoltz error: box:", shape=shape)
    for lo, hi in ((0.0, 0.0), (1.0, 0.0), (0.0, float("inf")), (float("nan"), 1.0)):
        for axis in range(3):
            box = unit.copy()
            box[2 * axis:2 * axis + 2] = lo, hi
            refused("WaveHoltz error: box:", box=box)
    refused("WaveHoltz error: box:", box=None)
    refused("WaveHoltz error: box:", nb=1)
    refused("WaveHoltz error: box:", nb=9)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        a = ones.copy()
        a[13] = bad
        refused("WaveHoltz error: box:", a=a)
    refused("WaveHoltz error: box:", a=None)
    refused("WaveHoltz error: box:", mask=64)
    refused("WaveHoltz error: box:", mask=-1)
    refused("WaveHoltz error: box:", shape=(40000, 40000, 40000), nb=2)  # stride Ly Lz beyond an int: refused before a is read
    refused("WaveHoltz error: time step:", ratio=257)
    refused("WaveHoltz error: time step:", ratio=-1)
    tiny = ones.copy()
    tiny[0] = 1e-3
    refused("WaveHoltz error: time step:", a=tiny, ratio=0)
    refused("WaveHoltz error: integrator:", integrator=2)
    refused("WaveHoltz error: integrator:", integrator=1, coarsen=17)
    refused("WaveHoltz error: integrator:", integrator=0, coarsen=2)
    refused("WaveHoltz error: omega", omega=0.0)
    # cuddh_wave_box_describe refuses the box by itself, and writes nothing
    for kw in (dict(shape=(0, 1, 1)), dict(nb=9), dict(mask=64), dict(a=np.where(np.arange(27) == 5, -1.0, 1.0))):
        args = {"shape": (1, 1, 1), "nb": 3, "a": ones, "mask": 63, **kw}
        err, D, dims, out, dos, sod = describe(args["shape"], unit.reshape(3, 2), args["nb"], args["a"], args["mask"])
        assert err != 0 and N.last_error().startswith("WaveHoltz error: box:"), kw
        assert dims.tolist() == [0, 0, 0, 0] and D.n_basis == 0 and all(np.isnan(v).all() for v in out.values()) and np.all(dos == -7) and np.all(sod == -7)


# ------------------------------------------------------------------ (e) the fixed point is the direct solve up to the time error
@pytest.mark.parametrize("scheme,coarsen", list(RECORDED_DISTANCE))
def test_fixed_point_is_the_direct_solve_up_to_the_time_error(scheme, coarsen):
    omega = math.pi
    B = wb.Box((2, 2, 2), ((-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0)), 3)
    M = B.model(omega, B.smooth_coefficient(), scheme, coarsen)
    f = B.example_load(omega)
    z, info = M.gmres(f, 20, 200, 1e-10)
    dist = wr.rel(M.solution(z), M.direct(f))
    print(f"{scheme}/{coarsen} on 2 x 2 x 2, n_basis 3, nt = {M.nt}: {info['num_matvec']} matvecs, distance to the direct solve {dist:.3e}")
    assert info["success"]
    assert dist < 2 * RECORDED_DISTANCE[scheme, coarsen]  # measured: 6.80e-4 (rk2), 1.40e-5 (rk4 / 4)
    x = np.random.default_rng(3).standard_normal(2 * M.n)
    assert wr.rel(M.period(x, f), M.period(x, None) + M.rhs(f)) < 1e-13
