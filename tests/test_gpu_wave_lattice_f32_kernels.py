"""kernels/wave_lattice_f32.hip, entry point by entry point through the C ABI, bit for bit against numpy.

The restatement is the one of test_gpu_wave_lattice_kernels.py (tables, line, stencil, the stages of test_gpu_wave_stage_kernels.py):
A holds integers in [-4, 4] and is not symmetric, the weights are 1 or 2, cx = 2, cy = 1/2, vectors hold integers in [-8, 8], invm
is 1/2, 1 or 2, Hi is 0, 1 or 2 and every coefficient is a power of two.  Every value the stencil and the stages form is then a
multiple of 2^-6 below 2^13: 19 bits, exact in float32 whatever the order of the operations.  The test asserts on the CPU that the
float64 restatement of the stencil and of every output survives a float32 round trip unchanged; it is then the expected float32
value bit for bit.  The description's tables are rounded from double sums (A[H][H] + A[0][0], w[H] + w[0]), integers here.

Lattices (nx, ny, n_basis) around the tile TX x TY read from cuddh_hip_wave32_tile_x / _y (128 x 16): (1,1,2); (3..6,1,2), whose
Lx = 4, 5, 6, 7 give all four paddings stride - Lx = 0, 3, 2, 1; (1,3,4) and (3,1,4), one element in a direction; (2,2,3), (3,2,5),
(2,3,6), (3,2,8); Lx = TX - 1, TX, TX + 1 at n_basis 2; at n_basis 4 (Lx = 3 nx + 1) the widths 124, 127 (with its padding column a
row of exactly TX floats) and 130 with Ly = 13, 16, 19; (43,27,4) with 12 tiles, more than eight and no multiple of it; Lx = TX + 1
at n_basis 5.  Forced and homogeneous form of all six stages.  Buffers are floats with a 16-element NaN-pattern guard on both
sides; after each call the guards, and every vector the stage does not write, are compared bitwise with what they held.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_wave_lattice_kernels import CX, CY, STAGES, description, host_vectors, stencil, tables
from test_gpu_wave_stage_kernels import CS, DT, FILT, HALF_DT, SN

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

GUARD = 16
PATTERN = 0x7FC0BEEF
ENTRY_POINTS = (*STAGES, "load", "begin", "store", "tile_x", "tile_y")


def tile():
    from cuddhelmholtz_amd import _native as N

    return N.lib.cuddh_hip_wave32_tile_x(), N.lib.cuddh_hip_wave32_tile_y()


def lattices():
    TX, TY = tile()
    n4, m4 = TX // 3, TY // 3  # n_basis 4: Lx = 3 n4 + 1 is the last width whose padded row fits one tile
    assert 3 * n4 + 1 <= TX < 3 * (n4 + 1) + 1 and 3 * m4 + 1 <= TY < 3 * (m4 + 1) + 1 and TX % 4 == 0
    around = [(n4 - 1, m4 - 1, 4), (n4, m4, 4), (n4 + 1, m4 + 1, 4), (n4, m4 - 1, 4), (n4 - 1, m4 + 1, 4)]
    many = (n4 + 1, 5 * m4 + 2, 4)  # two tiles by six at 128 x 16
    tiles = -(-(3 * many[0] + 1) // TX) * -(-(3 * many[1] + 1) // TY)
    assert tiles > 8 and tiles % 8 != 0, tiles
    assert 4 * (TX // 4) + 1 == TX + 1  # n_basis 5
    return [(1, 1, 2), (3, 1, 2), (4, 1, 2), (5, 1, 2), (6, 1, 2), (1, 3, 4), (3, 1, 4), (2, 2, 3), (3, 2, 5), (2, 3, 6), (3, 2, 8),
            (TX - 2, 1, 2), (TX - 1, 1, 2), (TX, 2, 2), *around, many, (TX // 4, 1, 5)]


def stride_of(nx, nb):
    return (nx * (nb - 1) + 1 + 3) // 4 * 4


class Buf32:
    """n floats at element offset `off` behind a 16-byte boundary, GUARD pattern elements on both sides"""

    def __init__(self, torch, dev, data, off=0):
        self.n, self.lo = len(data), GUARD + off
        host = np.full(self.lo + self.n + GUARD, PATTERN, dtype=np.uint32)
        host[self.lo:self.lo + self.n] = np.ascontiguousarray(data, dtype=np.float32).view(np.uint32)
        self.before = host.copy()
        self.t = torch.from_numpy(host.view(np.int32)).to(dev)
        assert self.t.data_ptr() % 16 == 0

    @property
    def p(self):
        return C.c_void_p(self.t.data_ptr() + 4 * self.lo)

    def bits(self):
        return self.t.cpu().numpy().view(np.uint32)

    def get(self):
        whole = self.bits()
        assert np.all(whole[:self.lo] == PATTERN), "elements before the vector were written"
        assert np.all(whole[self.lo + self.n:] == PATTERN), "elements behind the vector were written"
        return whole[self.lo:self.lo + self.n].view(np.float32).copy()

    def untouched(self):
        return np.array_equal(self.bits(), self.before)


def exact32(x, what):
    """x (float64) as float32, after asserting that nothing is lost"""
    y = np.ascontiguousarray(x, dtype=np.float64).astype(np.float32)
    assert np.array_equal(y.astype(np.float64), x), f"{what} is not exact in float32"
    return y


@functools.lru_cache(maxsize=None)
def case(nx, ny, nb, stencil_input):
    """(A, w, vectors with the stencil of `stencil_input` as "w"), computed once and never changed"""
    stride = stride_of(nx, nb)
    A, w = tables(nb, seed=nb)
    x = host_vectors(nx, ny, nb, stride, seed=1000 * nx + 10 * ny + nb)
    x["w"] = stencil(nx, ny, nb, stride, A, w, x[stencil_input])
    exact32(x["w"], "the stencil")
    for v in x.values():
        v.setflags(write=False)
    return A, w, x


def test_every_f32_entry_point_is_declared_and_no_other():
    from cuddhelmholtz_amd import _native as N

    declared = {s for s in N.declared_symbols() if s.startswith("cuddh_hip_wave32_")}
    assert declared == {f"cuddh_hip_wave32_{name}" for name in ENTRY_POINTS} and len(declared) == 11
    TX, TY = tile()
    assert TX % 4 == 0 and TX >= 8 and TY >= 4
    found = {(stride_of(nx, nb) - (nx * (nb - 1) + 1)) for nx, _, nb in lattices()}
    assert found == {0, 1, 2, 3}  # every padding


@pytest.mark.parametrize("name,forced", [(name, forced) for name in STAGES for forced in (True, False)],
                         ids=lambda v: v if isinstance(v, str) else ("forced" if v else "homogeneous"))
def test_f32_lattice_stage_matches_numpy_bit_for_bit(cuda, name, forced):
    import torch

    from cuddhelmholtz_amd import _native as N

    scalars, stencil_input, pointers, written, ref = STAGES[name]
    fn = getattr(N.lib, f"cuddh_hip_wave32_{name}")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for nx, ny, nb in lattices():
        stride = stride_of(nx, nb)
        A, w, x = case(nx, ny, nb, stencil_input)
        want = ref(x, forced)
        bufs = {v: Buf32(torch, cuda, exact32(x[v], v)) for v in pointers}
        args = [None if (v in ("F", "G") and not forced) else bufs[v].p for v in pointers]
        D = description(N, nx, ny, nb, stride, A, w)
        N.check(fn(C.byref(D), *scalars, *args, st), name)
        torch.cuda.synchronize()
        target = {buf: key for key, buf in written.items()}
        for v in pointers:
            where = f"{name} lattice=({nx},{ny},{nb}) stride={stride} {v}"
            if v in target:
                got = bufs[v].get()
                expected = exact32(want[target[v]], where)
                bad = np.flatnonzero(got.view(np.uint32) != expected.view(np.uint32))
                assert bad.size == 0, f"{where}: {bad.size} entries differ, the first at (I, J) = ({bad[0] % stride}, {bad[0] // stride}): " \
                                      f"{got[bad[0]]} for {expected[bad[0]]}"
            else:
                assert bufs[v].untouched(), where


@pytest.mark.parametrize("name", list(STAGES))
def test_f32_forced_form_with_zero_load_gives_the_homogeneous_bits(cuda, name):
    """on random float data, where every operation rounds"""
    import torch

    from cuddhelmholtz_amd import _native as N

    nx, ny, nb = 6, 7, 4
    Lx, Ly = nx * 3 + 1, ny * 3 + 1
    stride = stride_of(nx, nb)  # 20: one padding column
    rng = np.random.default_rng(3)
    A, w = rng.standard_normal((nb, nb)), rng.random(nb) + 0.5
    D = description(N, nx, ny, nb, stride, A, w)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _, _, pointers, written, _ = STAGES[name]
    scalars = {"rk2_a": (0.37, 0.8, -0.6), "rk2_b": (0.74, 0.8, -0.6, 0.013), "rk4_1": (0.37, 0.8, -0.6), "rk4_2": (0.37, 0.8, -0.6),
               "rk4_3": (0.74, 0.8, -0.6), "rk4_4": (0.1233, 0.8, -0.6, 0.013)}[name]
    x = {}
    for v in pointers:
        h = rng.standard_normal((Ly, stride)).astype(np.float32)
        h[:, Lx:] = 0.0
        x[v] = torch.from_numpy(h.reshape(-1)).to(cuda)
    outs = []
    for forced in (False, True):
        y = {v: t.clone() for v, t in x.items()}
        y["F"].zero_()
        y["G"].zero_()
        args = [None if (v in ("F", "G") and not forced) else C.c_void_p(y[v].data_ptr()) for v in pointers]
        N.check(getattr(N.lib, f"cuddh_hip_wave32_{name}")(C.byref(D), *scalars, *args, st), name)
        torch.cuda.synchronize()
        outs.append(y)
    for v in written.values():
        a, b = outs[0][v], outs[1][v]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and bool(torch.isfinite(a).all()), v
        assert not torch.equal(a, x[v]) and float(a.abs().max()) > 0, v
        assert float(a.view(Ly, stride)[:, Lx:].abs().max()) == 0.0  # the padding stays zero


def test_f32_bad_calls_are_refused_and_write_nothing(cuda):
    import torch

    from cuddhelmholtz_amd import _native as N

    nx, ny, nb = 2, 2, 4  # Lx = 7
    stride = 8
    A, w = tables(nb, seed=1)
    x = host_vectors(nx, 6, nb, 28, seed=5)  # 19 x 28 elements: room for every description tried, were one of them launched
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pointers = STAGES["rk4_2"][2]

    def attempt(D, swap=None, off=None, absent=()):
        bufs = {v: Buf32(torch, cuda, x[v], 1 if v == off else 0) for v in pointers}
        args = [None if v in absent else bufs[(swap or {}).get(v, v)].p for v in pointers]
        err = N.lib.cuddh_hip_wave32_rk4_2(C.byref(D), HALF_DT, CS, SN, *args, st)
        torch.cuda.synchronize()
        assert err == 1, (swap, off, absent, err)
        assert all(b.untouched() for b in bufs.values())

    good = description(N, nx, ny, nb, stride, A, w)
    attempt(good, swap={"ps_out": "ps"})  # an output equal to the stencil input
    attempt(good, off="q")  # a pointer off a 16-byte boundary (input)
    attempt(good, off="aq")  # ... (output)
    attempt(good, off="F")
    attempt(good, absent=("G",))  # F without G
    attempt(good, absent=("F",))
    attempt(good, absent=("p",))
    attempt(description(N, nx, ny, nb, 10, A, w))  # a stride >= Lx that is no multiple of 4 (the fp64 family takes it)
    attempt(description(N, nx, ny, nb, 7, A, w))
    attempt(description(N, nx, ny, nb, 4, A, w))  # a stride below Lx = 7
    attempt(description(N, nx, ny, 9, 28, A, w))  # n_basis beyond 8
    attempt(description(N, nx, ny, 1, 8, A, w))
    attempt(description(N, 0, ny, nb, stride, A, w))
    attempt(description(N, nx, -1, nb, stride, A, w))
    # rk2_b and rk4_4 write p, q, u, v: their stencil input cannot be one of them
    for name, scalars in (("rk2_b", (DT, CS, SN, FILT)), ("rk4_4", (DT, CS, SN, FILT))):
        bufs = {v: Buf32(torch, cuda, x[v]) for v in STAGES[name][2]}
        args = [bufs["q" if v == "ps" else v].p for v in STAGES[name][2]]
        assert getattr(N.lib, f"cuddh_hip_wave32_{name}")(C.byref(good), *scalars, *args, st) == 1
        torch.cuda.synchronize()
        assert all(b.untouched() for b in bufs.values())


def test_f32_load_begin_and_store_bit_for_bit(cuda):
    import torch

    from cuddhelmholtz_amd import _native as N

    rng = np.random.default_rng(9)
    ndof, n = 1501, 1620  # an odd ndof; 119 padding slots
    slot_of = rng.permutation(n)[:ndof].astype(np.int32)
    dof_of = np.full(n, -1, dtype=np.int32)
    dof_of[slot_of] = np.arange(ndof, dtype=np.int32)
    zu, zv = rng.standard_normal(ndof), rng.standard_normal(ndof)
    filt0 = 0.3  # rounded to float once, then one float product
    lat = lambda z: np.where(dof_of >= 0, z[np.maximum(dof_of, 0)].astype(np.float32), np.float32(0.0))  # noqa: E731
    d_dof, d_slot = torch.from_numpy(dof_of).to(cuda), torch.from_numpy(slot_of).to(cuda)
    d_zu, d_zv = (torch.from_numpy(np.concatenate([z, [np.nan]])).to(cuda) for z in (zu, zv))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    out = {v: Buf32(torch, cuda, np.full(n, 7.0)) for v in "pquvy"}
    N.check(N.lib.cuddh_hip_wave32_begin(n, filt0, ptr(d_dof), ptr(d_zu), ptr(d_zv), out["p"].p, out["q"].p, out["u"].p, out["v"].p, st), "begin")
    N.check(N.lib.cuddh_hip_wave32_load(n, ptr(d_dof), ptr(d_zv), out["y"].p, st), "load")
    torch.cuda.synchronize()
    f0 = np.float32(filt0)
    for v, want in (("p", lat(zu)), ("q", lat(zv)), ("u", f0 * lat(zu)), ("v", f0 * lat(zv)), ("y", lat(zv))):
        assert want.dtype == np.float32 and np.array_equal(out[v].get().view(np.uint32), want.view(np.uint32)), v
    assert float(np.abs(lat(zu)[dof_of < 0]).max()) == 0.0 and not np.array_equal(lat(zu).astype(np.float64)[slot_of], zu)  # it rounds
    # store: out of lattice order, float -> double, ndof entries and not one more
    src = Buf32(torch, cuda, rng.standard_normal(n).astype(np.float32))
    y = torch.full((ndof + 1,), -3.0, dtype=torch.float64, device=cuda)
    N.check(N.lib.cuddh_hip_wave32_store(ndof, ptr(d_slot), src.p, ptr(y), st), "store")
    torch.cuda.synchronize()
    want = src.get()[slot_of].astype(np.float64)
    got = y.cpu().numpy()
    assert np.array_equal(got[:ndof].view(np.uint64), want.view(np.uint64)) and got[ndof] == -3.0 and src.untouched()
