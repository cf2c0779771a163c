"""kernels/wave_box_f32.hip, entry point by entry point through the C ABI, bit for bit against numpy.

The inputs, the lattices and the restatement are those of tests/wave_box_f32_cases.py: `line`, `tables`, STAGES and the stage
references of the existing kernel tests, the stencil of include/cuddh_hip.h with an explicit stride (rows of a multiple of four
floats), integer non-symmetric tables and powers of two.  tests/test_wave_box_f32_host.py asserts on the CPU that the float64
restatement of the stencil and of every output survives a float32 round trip on every lattice and stage used here; it is then the
expected float32 value bit for bit, and no tolerance appears.

All six stages, forced (F, G given) and homogeneous (both NULL).  Buffers are floats with a 16-element NaN-pattern guard on both
sides; after each call the guards, and every vector the stage does not write, are compared bitwise with what they held.  The same
call twice gives the same bits; the forced form with zero load gives the homogeneous bits on random reals (compile-time n_basis 4
and 5 and the run-time form); every refusal returns 1 and writes nothing.
"""
import ctypes as C

import numpy as np
import pytest

import wave_box_f32_cases as cases
from test_gpu_wave_lattice_f32_kernels import Buf32
from test_gpu_wave_lattice_kernels import STAGES
from test_gpu_wave_stage_kernels import CS, DT, FILT, HALF_DT, SN

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]


def description(N, nx, ny, nz, nb, stride, A, w):
    D = N.WaveBox()
    D.nx, D.ny, D.nz, D.n_basis, D.stride, D.cx, D.cy, D.cz = nx, ny, nz, nb, stride, cases.CX, cases.CY, cases.CZ
    for i, a in enumerate(A.reshape(-1)):
        D.A[i] = a
    for i, a in enumerate(w):
        D.w[i] = a
    return D


@pytest.mark.parametrize("name,forced", [(name, forced) for name in STAGES for forced in (True, False)],
                         ids=lambda v: v if isinstance(v, str) else ("forced" if v else "homogeneous"))
def test_f32_box_stage_matches_numpy_bit_for_bit(cuda, name, forced):
    import torch

    from cuddhelmholtz_amd import _native as N

    scalars, stencil_input, pointers, written, _ = STAGES[name]
    fn = getattr(N.lib, f"cuddh_hip_wave_box32_{name}")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    target = {buf: key for key, buf in written.items()}
    repeated = 0
    for lat in cases.lattices():
        Lx, Ly, Lz, stride = cases.dims(*lat)
        A, w, x = cases.case(lat, stencil_input)
        want = cases.expected(lat, name, forced)
        D = description(N, *lat, stride, A, w)

        def run():
            bufs = {v: Buf32(torch, cuda, cases.exact32(x[v], v)) for v in pointers}
            args = [None if (v in ("F", "G") and not forced) else bufs[v].p for v in pointers]
            N.check(fn(C.byref(D), *scalars, *args, st), name)
            torch.cuda.synchronize()
            return bufs

        bufs = run()
        for v in pointers:
            where = f"{name} lattice={lat} stride={stride} {v}"
            if v in target:
                got = bufs[v].get()
                expected = cases.exact32(want[target[v]], where)
                bad = np.flatnonzero(got.view(np.uint32) != expected.view(np.uint32))
                assert bad.size == 0, f"{where}: {bad.size} entries differ, the first at (I, J, K) = ({bad[0] % stride}, " \
                                      f"{bad[0] // stride % Ly}, {bad[0] // (stride * Ly)}): {got[bad[0]]} for {expected[bad[0]]}"
            else:
                assert bufs[v].untouched(), where
        if lat == (2, 2, 2, 3) or cases.workgroups(lat) > 8:  # the same call on the same inputs again: the same bits
            again = run()
            repeated += 1
            for v in pointers:
                assert np.array_equal(again[v].bits(), bufs[v].bits()), f"{name} lattice={lat} {v}: a second call gave other bits"
    assert repeated >= 2


SCALARS = {"rk2_a": (0.37, 0.8, -0.6), "rk2_b": (0.74, 0.8, -0.6, 0.013), "rk4_1": (0.37, 0.8, -0.6), "rk4_2": (0.37, 0.8, -0.6),
           "rk4_3": (0.74, 0.8, -0.6), "rk4_4": (0.1233, 0.8, -0.6, 0.013)}


@pytest.mark.parametrize("name", list(STAGES))
def test_f32_box_forced_form_with_zero_load_gives_the_homogeneous_bits(cuda, name):
    """on random float data, where every operation rounds: n_basis 4 and 5 (compile-time) and 3 (run-time)"""
    import torch

    from cuddhelmholtz_amd import _native as N

    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _, _, pointers, written, _ = STAGES[name]
    for lat in ((4, 3, 2, 4), (3, 2, 2, 5), (3, 2, 3, 3)):
        nb = lat[3]
        Lx, Ly, Lz, stride = cases.dims(*lat)
        assert stride > Lx  # with padding columns
        rng = np.random.default_rng(3)
        A, w = rng.standard_normal((nb, nb)), rng.random(nb) + 0.5
        D = description(N, *lat, stride, A, w)
        D.cx, D.cy, D.cz = 0.7, 1.3, 2.1
        x = {}
        for v in pointers:
            h = rng.standard_normal((Lz, Ly, stride)).astype(np.float32)
            h[:, :, Lx:] = 0.0
            x[v] = torch.from_numpy(h.reshape(-1)).to(cuda)
        outs = []
        for forced in (False, True, True):
            y = {v: t.clone() for v, t in x.items()}
            y["F"].zero_()
            y["G"].zero_()
            args = [None if (v in ("F", "G") and not forced) else C.c_void_p(y[v].data_ptr()) for v in pointers]
            N.check(getattr(N.lib, f"cuddh_hip_wave_box32_{name}")(C.byref(D), *SCALARS[name], *args, st), name)
            torch.cuda.synchronize()
            outs.append(y)
        for v in written.values():
            a, b, c = (o[v].view(torch.int32) for o in outs)
            assert torch.equal(a, b) and torch.equal(b, c) and bool(torch.isfinite(outs[0][v]).all()), (lat, v)
            assert not torch.equal(outs[0][v], x[v]) and float(outs[0][v].abs().max()) > 0, (lat, v)
            assert float(outs[0][v].view(Lz, Ly, stride)[:, :, Lx:].abs().max()) == 0.0  # the padding stays zero


def test_f32_box_bad_calls_are_refused_and_write_nothing(cuda):
    import torch

    from cuddhelmholtz_amd import _native as N

    from test_gpu_wave_lattice_kernels import tables

    lat = (2, 2, 2, 4)  # Lx = Ly = Lz = 7
    nb, stride = 4, 8
    A, w = tables(nb, seed=1)
    x = cases.host_vectors(2, 6, 6, nb, 28, seed=5)  # 28 x 19 x 19 elements: room for every description tried, were one of them launched
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pointers = STAGES["rk4_2"][2]

    def attempt(D, swap=None, off=None, shift=1, absent=()):
        bufs = {v: Buf32(torch, cuda, x[v], shift if v == off else 0) for v in pointers}
        args = [None if v in absent else bufs[(swap or {}).get(v, v)].p for v in pointers]
        err = N.lib.cuddh_hip_wave_box32_rk4_2(None if D is None else C.byref(D), HALF_DT, CS, SN, *args, st)
        torch.cuda.synchronize()
        assert err == 1, (swap, off, shift, absent, err)
        assert all(b.untouched() for b in bufs.values())

    good = description(N, *lat, stride, A, w)
    attempt(good, swap={"ps_out": "ps"})  # an output equal to the stencil input
    for shift in (1, 2, 3):  # a pointer off a 16-byte boundary by 1, 2 and 3 floats: an input, an output, the stencil input, the load
        for v in ("q", "aq", "ps", "F", "G", "ps_out", "invm"):
            attempt(good, off=v, shift=shift)
    attempt(good, absent=("G",))  # F without G
    attempt(good, absent=("F",))
    for v in pointers:  # a NULL vector
        if v not in ("F", "G"):
            attempt(good, absent=(v,))
    attempt(None)  # no description
    attempt(description(N, 2, 2, 2, nb, 10, A, w))  # a stride >= Lx that is even and no multiple of 4 (the fp64 family takes it)
    attempt(description(N, 2, 2, 2, nb, 7, A, w))  # Lx itself
    attempt(description(N, 2, 2, 2, nb, 9, A, w))
    attempt(description(N, 2, 2, 2, nb, 4, A, w))  # a multiple of 4 below Lx = 7
    attempt(description(N, 2, 2, 2, nb, 0, A, w))
    attempt(description(N, 2, 2, 2, 9, 20, A, w))  # n_basis beyond 8
    attempt(description(N, 2, 2, 2, 1, stride, A, w))  # and below 2
    for bad in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (2, 2, -1), (-1, 2, 2)):
        attempt(description(N, *bad, nb, stride, A, w))
    attempt(description(N, 2, 40000, 40000, nb, stride, A, w))  # stride Ly Lz beyond an int
    attempt(description(N, 2, 5461, 5461, nb, stride, A, w))  # 8 * 16384 * 16384 = 2^31: one beyond
    # rk2_b and rk4_4 write p, q, u, v: their stencil input cannot be one of them
    for name, scalars in (("rk2_b", (DT, CS, SN, FILT)), ("rk4_4", (DT, CS, SN, FILT))):
        for out in "pquv":
            bufs = {v: Buf32(torch, cuda, x[v]) for v in STAGES[name][2]}
            args = [bufs[out if v == "ps" else v].p for v in STAGES[name][2]]
            assert getattr(N.lib, f"cuddh_hip_wave_box32_{name}")(C.byref(good), *scalars, *args, st) == 1
            torch.cuda.synchronize()
            assert all(b.untouched() for b in bufs.values())
