"""The host side of the fp32 box sweeps: cuddh_wave_box_describe_rows, the new symbols, the refusals of the precision
argument, and the exactness in float32 of everything tests/test_gpu_wave_box_f32_kernels.py compares bit for bit.  No GPU.

(a) cuddh_wave_box_describe_rows with a row multiple of 4: stride % 4 == 0 and stride - Lx in {0, 1, 2, 3}, all four paddings at
    n_basis 2 (nx = 3, 4, 5, 6: Lx = 4, 5, 6, 7); the slot maps are inverse to each other with -1 in the padding; m, h, invm, Hi are
    those of cuddh_wave_box_describe.  With 2 it is that call array for array.  3 is refused ("WaveHoltz error: box:"), nothing written.
(b) The new symbols are declared and are functions; none of them carries a prefix that an existing test pins.
(c) precision "f16", 32 or None is a ValueError before any native call; precision code 2 through cuddh_waveholtz_box_create_precision
    returns NULL with "WaveHoltz error: precision:".
(d) For every lattice and stage of the kernel test the float64 restatement of the stencil and of every output survives a float32
    round trip, so it IS the expected float32 value; the largest magnitude is printed.  No tolerance anywhere.
"""
import ctypes as C

import numpy as np
import pytest

import wave_box_f32_cases as cases
from test_gpu_wave_lattice_kernels import STAGES

BOX3 = ((-1.0, 0.5), (0.25, 1.0), (-0.5, 1.5))
REALS = ("m", "h", "invm", "Hi")


def describe(shape, nb, rows, a=None, mask=63, box=BOX3):
    """cuddh_wave_box_describe_rows (rows = None: cuddh_wave_box_describe) into arrays pre-filled with markers, sized for a stride of
    Lx + 3 whatever the call does"""
    from cuddhelmholtz_amd import _native as N

    L = [n * (nb - 1) + 1 for n in shape]
    n = L[0] * L[1] * L[2]
    D, dims = N.WaveBox(), np.full(4, -7, dtype=np.int32)
    out = {k: np.full(n, np.nan) for k in REALS}
    dos, sod = np.full((L[0] + 3) * L[1] * L[2], -7, dtype=np.int32), np.full(n, -7, dtype=np.int32)
    flat = np.ascontiguousarray(box, dtype=np.float64).reshape(-1)
    head = (*shape, flat.ctypes.data, nb, None if a is None else a.ctypes.data, mask)
    tail = (C.byref(D), dims.ctypes.data, *[out[k].ctypes.data for k in REALS], dos.ctypes.data, sod.ctypes.data)
    err = N.lib.cuddh_wave_box_describe(*head, *tail) if rows is None else N.lib.cuddh_wave_box_describe_rows(*head, rows, *tail)
    return err, D, dims, out, dos, sod


def same_description(D, E):
    """field by field, bit for bit (the struct's padding bytes say nothing)"""
    fields = lambda X: (X.nx, X.ny, X.nz, X.n_basis, X.stride, np.array([X.cx, X.cy, X.cz, *X.A, *X.w]).tobytes())  # noqa: E731
    return fields(D) == fields(E)


@pytest.mark.parametrize("shape,nb", [((3, 1, 1), 2), ((4, 2, 1), 2), ((5, 1, 2), 2), ((6, 1, 1), 2), ((2, 2, 2), 3), ((1, 2, 3), 4), ((2, 1, 1), 5),
                                      ((1, 1, 2), 8)])
def test_describe_rows_of_four(shape, nb):
    Lx, Ly, Lz = (n * (nb - 1) + 1 for n in shape)
    n = Lx * Ly * Lz
    a = 0.5 + np.random.default_rng(nb).random(n)
    err, D, dims, out, dos, sod = describe(shape, nb, 4, a)
    assert err == 0
    stride = int(dims[3])
    assert stride % 4 == 0 and stride - Lx in (0, 1, 2, 3) and stride == (Lx + 3) // 4 * 4
    assert dims.tolist() == [Lx, Ly, Lz, stride] and (D.nx, D.ny, D.nz, D.n_basis, D.stride) == (*shape, nb, stride)
    # the slot maps: node (I, J, K) at I + stride (J + Ly K); inverse to each other, -1 in the padding, nothing written behind
    slots = stride * Ly * Lz
    g = np.arange(n)
    assert np.array_equal(sod, g % Lx + stride * (g // Lx))
    assert np.array_equal(dos[sod], g) and np.count_nonzero(dos[:slots] == -1) == (stride - Lx) * Ly * Lz
    inside = dos[:slots] >= 0
    assert np.array_equal(sod[dos[:slots][inside]], np.flatnonzero(inside)) and np.all(dos[slots:] == -7)
    assert np.all((np.arange(slots) % stride >= Lx) == ~inside)
    # everything but the stride is the existing call's
    err2, D2, dims2, out2, _, _ = describe(shape, nb, None, a)
    assert err2 == 0 and dims2[:3].tolist() == [Lx, Ly, Lz] and int(dims2[3]) == Lx + Lx % 2
    for k in REALS:
        assert np.array_equal(out[k], out2[k]) and np.all(np.isfinite(out[k])), k
    D2.stride = stride
    assert same_description(D, D2)


def test_the_four_paddings_at_n_basis_2():
    found = set()
    for nx in (3, 4, 5, 6):
        err, _, dims, *_ = describe((nx, 1, 1), 2, 4)
        assert err == 0
        found.add(int(dims[3]) - int(dims[0]))
    assert found == {0, 1, 2, 3}


@pytest.mark.parametrize("shape,nb", [((3, 1, 1), 2), ((4, 2, 1), 2), ((2, 2, 2), 3), ((1, 2, 3), 4), ((2, 1, 1), 5)])
@pytest.mark.parametrize("mask", [0, 63, 1])
def test_describe_rows_of_two_is_the_existing_call(shape, nb, mask):
    n = int(np.prod([k * (nb - 1) + 1 for k in shape]))
    a = 0.5 + np.random.default_rng(7).random(n)
    new, old = describe(shape, nb, 2, a, mask), describe(shape, nb, None, a, mask)
    assert new[0] == 0 and old[0] == 0
    assert same_description(new[1], old[1]) and np.array_equal(new[2], old[2])
    for k in REALS:
        assert np.array_equal(new[3][k], old[3][k]), k
    assert np.array_equal(new[4], old[4]) and np.array_equal(new[5], old[5])


@pytest.mark.parametrize("rows", [3, 0, 1, 8, -4])
def test_any_other_row_multiple_is_refused_and_nothing_is_written(rows):
    from cuddhelmholtz_amd import _native as N

    err, D, dims, out, dos, sod = describe((2, 2, 2), 3, rows, np.ones(125))
    assert err != 0 and N.last_error().startswith("WaveHoltz error: box:"), N.last_error()
    assert dims.tolist() == [-7] * 4 and D.n_basis == 0 and D.stride == 0 and all(np.isnan(v).all() for v in out.values())
    assert np.all(dos == -7) and np.all(sod == -7)


def test_the_int_check_uses_the_padded_stride():
    from cuddhelmholtz_amd import _native as N

    # Lx = 5, Ly = Lz = 16384: the stride of 6 of rows of two gives 6 * 2^28 slots, which fit in an int (that description is not
    # built here: it would be); the stride of 8 of rows of four gives 2^31, which do not
    unit = np.array([0.0, 1.0, 0.0, 1.0, 0.0, 1.0])
    err = N.lib.cuddh_wave_box_describe_rows(4, 16383, 16383, unit.ctypes.data, 2, None, 63, 4, None, None, None, None, None, None, None, None)
    assert err != 0 and N.last_error().startswith("WaveHoltz error: box:") and "8 x 16384 x 16384 slots does not fit" in N.last_error()


def test_the_new_symbols_are_declared_and_are_functions():
    from cuddhelmholtz_amd import _native as N

    declared = set(N.declared_symbols())
    kernels = {f"cuddh_hip_wave_box32_{name}" for name in STAGES} | {f"cuddh_hip_wave_box32_tile_{a}" for a in "xyz"}
    assert {s for s in declared if s.startswith("cuddh_hip_wave_box32_")} == kernels
    new = kernels | {"cuddh_waveholtz_box_create_precision", "cuddh_waveholtz_box_precision", "cuddh_wave_box_describe_rows"}
    assert new <= declared
    for s in new:
        assert isinstance(getattr(N.lib, s), C._CFuncPtr), s
    pinned = ("cuddh_hip_wave_box_", "cuddh_hip_wave32_", "cuddh_hip_wave_lattice_", "cuddh_hip_wave_stage_", "cuddh_hip_wave_cells", "cuddh_hip_wave_weights")
    assert not any(s.startswith(pinned) for s in new)
    TX, TY, TZ = cases.tile()
    assert TX % 4 == 0 and TX >= 8 and TY >= 1 and TZ >= 1


GOOD = dict(omega=1.0, h_a=np.ones(8), shape=(1, 1, 1), box=((0, 1), (0, 1), (0, 1)), n_basis=2)


@pytest.mark.parametrize("precision", ["f16", 32, None, "F32", 1.0, b"f32"])
def test_a_bad_precision_raises_before_any_native_call(monkeypatch, precision):
    import cuddhelmholtz_amd as cd

    class NoLibrary:  # any native call fails the test with another exception
        def __getattr__(self, name):
            raise AssertionError(f"{name} was called before the arguments were checked")

    monkeypatch.setattr(cd.api, "lib", NoLibrary())
    with pytest.raises(ValueError, match="precision"):
        cd.WaveHoltzBox(**GOOD, precision=precision)


def test_the_padded_size_check_uses_the_stride_of_the_precision(monkeypatch):
    import cuddhelmholtz_amd as cd

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was called before the arguments were checked")

    monkeypatch.setattr(cd.api, "lib", NoLibrary())
    # Lx = 5, Ly = Lz = 16384: 6 * 2^28 slots fit in an int, 8 * 2^28 do not; h_a is looked at after the size
    with pytest.raises(ValueError, match="padded lattice of 8 x 16384 x 16384 slots does not fit"):
        cd.WaveHoltzBox(1.0, np.ones(1), shape=(4, 16383, 16383), box=GOOD["box"], n_basis=2, precision="f32")
    with pytest.raises(ValueError, match="h_a must have shape"):
        cd.WaveHoltzBox(1.0, np.ones(1), shape=(4, 16383, 16383), box=GOOD["box"], n_basis=2)


def test_a_bad_precision_code_is_refused_by_the_library():
    from cuddhelmholtz_amd import _native as N

    unit, ones = np.array([0.0, 1.0, 0.0, 1.0, 0.0, 1.0]), np.ones(27)
    for code in (2, -1, 7):
        h = N.lib.cuddh_waveholtz_box_create_precision(1.0, 1, 1, 1, unit.ctypes.data, 3, ones.ctypes.data, 0, 1, 1, 63, code)
        assert not h and N.last_error().startswith("WaveHoltz error: precision:"), N.last_error()
    # the box's own refusals keep their prefix at either precision
    for code in (0, 1):
        h = N.lib.cuddh_waveholtz_box_create_precision(1.0, 0, 1, 1, unit.ctypes.data, 3, ones.ctypes.data, 0, 1, 1, 63, code)
        assert not h and N.last_error().startswith("WaveHoltz error: box:")
    assert N.lib.cuddh_waveholtz_box_precision(None) == -1


def test_every_input_and_output_of_the_kernel_test_is_exact_in_float32():
    found = cases.lattices()
    TX, TY, TZ = cases.tile()
    assert {cases.dims(*lat)[3] - cases.dims(*lat)[0] for lat in found if lat[3] == 2} == {0, 1, 2, 3}  # every padding
    for axis, T in enumerate((TX, TY, TZ)):
        assert {max(2, T - 1), max(2, T), T + 1} <= {cases.dims(*lat)[axis] for lat in found if lat[3] == 2}
    assert any(cases.workgroups(lat) > 8 and cases.workgroups(lat) % 8 != 0 for lat in found if lat[3] == 4)
    assert {lat[3] for lat in found} == {2, 3, 4, 5, 6, 8}
    largest = 0.0
    for lat in found:
        for name, (_, stencil_input, pointers, written, _) in STAGES.items():
            A, w, x = cases.case(lat, stencil_input)
            cases.exact32(x["w"], f"the stencil of {stencil_input} on {lat}")
            assert np.any(x["w"] != 0)
            for v in pointers:
                cases.exact32(x[v], f"{v} on {lat}")
            for forced in (True, False):
                want = cases.expected(lat, name, forced)
                assert set(want) == set(written)
                for key, vec in want.items():
                    cases.exact32(vec, f"{name} {'forced' if forced else 'homogeneous'} {key} on {lat}")
                    largest = max(largest, float(np.abs(vec).max()), float(np.abs(x["w"]).max()))
    print(f"fp32 box kernel test: {len(found)} lattices, largest magnitude {largest:g}, all exact in float32")
    assert largest < 2.0 ** 24
