"""kernels/wave_pair.hip and wave_pair_f32.hip (two lattice sweeps per launch), entry point by entry point through the C ABI.

(a) Against numpy, bit for bit.  Tables, vectors and scalars are those of test_gpu_wave_lattice_kernels.py: A holds integers in
[-4, 4] and is not symmetric, weights 1 or 2, cx = 2, cy = 1/2, vectors integers in [-8, 8], invm 1/2, 1 or 2, Hi 0, 1 or 2, every
scalar a power of two (the two sweeps of a pair get different c, s, so that a swapped pair of scalars shows).  The expected
values are tests/wave_pair_reference.py, which states each pair from its pointwise table.  Before anything is compared the test
asserts, in numpy, that the whole chain of a pair is exact: the float64 run equals a longdouble run with the stencil summed in the
reversed order, and for the fp32 family it also equals a run in float32 (one rounding per operation, more than the kernel's fused
ones).  A pair chains two stencils and two stages; at these magnitudes its values still fit float32's 24 bits on every lattice
of the list (asserted here, on the CPU side, case by case), so both families take the same vectors.

(b) Against the existing launches, bit for bit, on random reals (standard_normal vectors, tables and non-dyadic scalars; padding
columns zero, invm = 0 there): the paired launch on one copy, the two one-sweep entry points (cuddh_hip_wave_lattice_*_f64,
cuddh_hip_wave32_*) in the march's order on another; every output must be equal as bit patterns.  This is the gate on the order
of operations.

Lattices (nx, ny, n_basis) are built from the tile the library reports (cuddh_hip_wave_pair_tile_x / _y, _tile_y_run_time for the
run-time n_basis instantiation of the fp64 family): (1,1,2); (1,3,4), (3,1,4); (2,2,3); (3,2,5); (2,3,6), (3,2,8) on the run-time
instantiation; n_basis 4 with widths one element short of a tile, exactly a tile with its padding, two nodes into a second tile and
heights one row block short, exactly a tile, one row block over; Lx = TX - 1, TX, TX + 1 at n_basis 2; Ly = TYr, TYr + 1 at
n_basis 2 (TYr the run-time form's rows); Lx = TX + 1 at n_basis 5; one lattice of more than eight tiles, no multiple of eight;
for fp32 every row padding 0, 1, 2, 3.  Forced and homogeneous forms.  Buffers carry a 16-element NaN-pattern guard on both
sides; after each call the guards and every vector the launch does not write are compared bitwise.  The hazards of the header
(an output that is read with a halo), F without G, a stride of the wrong multiple and a misaligned pointer return an error and
write nothing.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import wave_pair_reference as wp
from test_gpu_wave_lattice_f32_kernels import Buf32
from test_gpu_wave_lattice_kernels import description, host_vectors, tables
from test_gpu_wave_stage_kernels import DT, FILT, HALF_DT, SIXTH_DT, Buf

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

C0, S0, C1, S1, C2, S2 = 2.0, -4.0, -1.0, 2.0, 4.0, -2.0

# name -> (scalars, pointer arguments in the entry point's order, {reference name: buffer written}, numpy restatement)
KINDS = {
    "rk2": ((HALF_DT, DT, C0, S0, C1, S1, FILT), ("p", "q", "invm", "Hi", "F", "G", "p_out", "q_out", "u", "v"),
            {"p": "p_out", "q": "q_out", "u": "u", "v": "v"}, wp.pair_rk2),
    "rk4_12": ((HALF_DT, C0, S0, C1, S1), ("p", "q", "invm", "Hi", "F", "G", "ps2", "qs", "aq", "ap"),
               {v: v for v in ("ps2", "qs", "aq", "ap")}, wp.pair_rk4_12),
    "rk4_34": ((DT, SIXTH_DT, C1, S1, C2, S2, FILT), ("ps2", "p", "qs", "aq", "ap", "invm", "Hi", "F", "G", "p_out", "q", "u", "v"),
               {"p": "p_out", "q": "q", "u": "u", "v": "v"}, wp.pair_rk4_34),
}
# the same pairs on random reals: non-dyadic scalars, and the two one-sweep calls a pair stands for
REAL = dict(half_dt=0.0171, dt=0.031, sixth_dt=0.0049, c0=0.8, s0=-0.6, c1=0.3, s1=0.95, c2=-0.5, s2=0.86, filt=0.013)
REAL_SCALARS = {"rk2": ("half_dt", "dt", "c0", "s0", "c1", "s1", "filt"), "rk4_12": ("half_dt", "c0", "s0", "c1", "s1"),
                "rk4_34": ("dt", "sixth_dt", "c1", "s1", "c2", "s2", "filt")}
SWEEPS = {
    "rk2": [("rk2_a", ("half_dt", "c0", "s0"), ("p", "q", "invm", "Hi", "F", "G", "qs", "ps")),
            ("rk2_b", ("dt", "c1", "s1", "filt"), ("ps", "qs", "invm", "Hi", "F", "G", "p", "q", "u", "v"))],
    "rk4_12": [("rk4_1", ("half_dt", "c0", "s0"), ("p", "q", "invm", "Hi", "F", "G", "ps", "qs", "aq", "ap")),
               ("rk4_2", ("half_dt", "c1", "s1"), ("ps", "p", "q", "invm", "Hi", "F", "G", "ps2", "qs", "aq", "ap"))],
    "rk4_34": [("rk4_3", ("dt", "c1", "s1"), ("ps2", "p", "q", "invm", "Hi", "F", "G", "ps", "qs", "aq", "ap")),
               ("rk4_4", ("sixth_dt", "c2", "s2", "filt"), ("ps", "qs", "aq", "ap", "invm", "Hi", "F", "G", "p", "q", "u", "v"))],
}
ALL = ("p", "q", "u", "v", "ps", "ps2", "qs", "aq", "ap", "F", "G", "invm", "Hi", "p_out", "q_out")

FAMILIES = {
    "f64": dict(pair="cuddh_hip_wave_pair_{}_f64", sweep="cuddh_hip_wave_lattice_{}_f64", tile="cuddh_hip_wave_pair_tile_", multiple=2, buf=Buf,
                dtype=np.float64, bits=np.uint64),
    "f32": dict(pair="cuddh_hip_wave_pair32_{}", sweep="cuddh_hip_wave32_{}", tile="cuddh_hip_wave_pair32_tile_", multiple=4, buf=Buf32,
                dtype=np.float32, bits=np.uint32),
}


def tiles(family):
    """(TX, TY, TY of the run-time n_basis instantiation)"""
    from cuddhelmholtz_amd import _native as N

    t = FAMILIES[family]["tile"]
    TX, TY = getattr(N.lib, t + "x")(), getattr(N.lib, t + "y")()
    return TX, TY, N.lib.cuddh_hip_wave_pair_tile_y_run_time() if family == "f64" else TY


def stride_of(family, nx, nb):
    m = FAMILIES[family]["multiple"]
    return -(-(nx * (nb - 1) + 1) // m) * m


def lattices(family):
    TX, TY, TYR = tiles(family)
    n4, m4 = TX // 3, TY // 3  # n_basis 4: Lx = 3 n4 + 1 is the last width whose padded row fits one tile
    assert 3 * n4 + 1 <= TX < 3 * (n4 + 1) + 1 and 3 * m4 + 1 <= TY < 3 * (m4 + 1) + 1 and TX % 4 == 0 and TYR >= 2
    around = [(n4 - 1, m4 - 1, 4), (n4, m4, 4), (n4 + 1, m4 + 1, 4), (n4, m4 - 1, 4), (n4 - 1, m4 + 1, 4)]
    many = (n4 + 1, 5 * m4 + 2, 4)
    n_tiles = -(-(3 * many[0] + 1) // TX) * -(-(3 * many[1] + 1) // TY)
    assert n_tiles > 8 and n_tiles % 8 != 0, n_tiles
    assert 4 * (TX // 4) + 1 == TX + 1  # n_basis 5
    out = [(1, 1, 2), (1, 3, 4), (3, 1, 4), (2, 2, 3), (3, 2, 5), (2, 3, 6), (3, 2, 8), (TX - 2, 1, 2), (TX - 1, 1, 2), (TX, 2, 2),
           (1, TYR - 1, 2), (2, TYR, 2), *around, many, (TX // 4, 1, 5)]
    if family == "f32":
        out += [(3, 1, 2), (4, 1, 2), (5, 1, 2), (6, 1, 2)]
        assert {stride_of(family, nx, nb) - (nx * (nb - 1) + 1) for nx, _, nb in out} == {0, 1, 2, 3}  # every padding
    return out


@functools.lru_cache(maxsize=None)
def exact_case(family, nx, ny, nb, kind, forced):
    """(A, w, inputs, expected outputs) in float64, computed once and never changed; asserts that the chain is exact"""
    stride = stride_of(family, nx, nb)
    A, w = tables(nb, seed=nb)
    h = host_vectors(nx, ny, nb, stride, seed=1000 * nx + 10 * ny + nb)
    x = {**h, "ps2": h["ps"], "p_out": h["ps_out"], "q_out": h["ps_out"][::-1].copy()}
    scalars, _, _, ref = KINDS[kind]
    want = ref(wp.stiffness(nx, ny, nb, stride, A, w), x, *scalars, forced)
    # exact in float64: a longdouble run with the stencil summed backwards gives the same values
    wide = ref(wp.stiffness(nx, ny, nb, stride, A, w, dtype=np.longdouble, reverse=True), {k: v.astype(np.longdouble) for k, v in x.items()}, *scalars, forced)
    for k, v in want.items():
        assert v.dtype == np.float64 and wide[k].dtype == np.longdouble
        assert np.array_equal(v.astype(np.longdouble), wide[k]), f"{kind} ({nx},{ny},{nb}) {k}: the chain is not exact in float64"
    if family == "f32":
        narrow = ref(wp.stiffness(nx, ny, nb, stride, A, w, dtype=np.float32), {k: v.astype(np.float32) for k, v in x.items()}, *scalars, forced)
        for k, v in want.items():
            assert narrow[k].dtype == np.float32
            assert np.array_equal(narrow[k].astype(np.float64), v), f"{kind} ({nx},{ny},{nb}) {k}: the chain is not exact in float32"
    for v in (*x.values(), *want.values()):
        v.setflags(write=False)
    return A, w, x, want


def test_every_pair_entry_point_is_declared():
    from cuddhelmholtz_amd import _native as N

    declared = set(N.declared_symbols())
    for family, f in FAMILIES.items():
        for kind in KINDS:
            assert f["pair"].format(kind) in declared
        TX, TY, TYR = tiles(family)
        assert TX % 4 == 0 and TX >= 8 and TY >= 4 and 2 <= TYR <= TY
        lattices(family)  # its assertions


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("kind,forced", [(kind, forced) for kind in KINDS for forced in (True, False)],
                         ids=lambda v: v if isinstance(v, str) else ("forced" if v else "homogeneous"))
def test_pair_matches_numpy_bit_for_bit(cuda, family, kind, forced):
    import torch

    from cuddhelmholtz_amd import _native as N

    f = FAMILIES[family]
    scalars, pointers, written, _ = KINDS[kind]
    fn = getattr(N.lib, f["pair"].format(kind))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    target = {buf: key for key, buf in written.items()}
    for nx, ny, nb in lattices(family):
        stride = stride_of(family, nx, nb)
        A, w, x, want = exact_case(family, nx, ny, nb, kind, forced)
        bufs = {v: f["buf"](torch, cuda, x[v], 0) for v in pointers}
        args = [None if (v in ("F", "G") and not forced) else bufs[v].p for v in pointers]
        D = description(N, nx, ny, nb, stride, A, w)
        N.check(fn(C.byref(D), *scalars, *args, st), kind)
        torch.cuda.synchronize()
        for v in pointers:
            where = f"{family} {kind} lattice=({nx},{ny},{nb}) stride={stride} {v}"
            if v in target:
                got = bufs[v].get()
                expected = np.ascontiguousarray(want[target[v]]).astype(f["dtype"])
                assert np.array_equal(expected.astype(np.float64), want[target[v]]), where
                bad = np.flatnonzero(got.view(f["bits"]) != expected.view(f["bits"]))
                assert bad.size == 0, f"{where}: {bad.size} entries differ, the first at (I, J) = ({bad[0] % stride}, {bad[0] // stride}): " \
                                      f"{got[bad[0]]} for {expected[bad[0]]}"
            else:
                assert bufs[v].untouched(), where


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("kind,forced", [(kind, forced) for kind in KINDS for forced in (True, False)],
                         ids=lambda v: v if isinstance(v, str) else ("forced" if v else "homogeneous"))
def test_pair_gives_the_bits_of_the_two_sweeps_on_random_reals(cuda, family, kind, forced):
    import torch

    from cuddhelmholtz_amd import _native as N

    f = FAMILIES[family]
    _, pointers, written, _ = KINDS[kind]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    integer = torch.int64 if family == "f64" else torch.int32
    for nx, ny, nb in lattices(family):
        Lx, Ly, stride = nx * (nb - 1) + 1, ny * (nb - 1) + 1, stride_of(family, nx, nb)
        rng = np.random.default_rng(100 * nx + 10 * ny + nb)
        A, w = rng.standard_normal((nb, nb)), rng.random(nb) + 0.5
        D = description(N, nx, ny, nb, stride, A, w)
        x = {}
        for v in ALL:
            h = rng.standard_normal((Ly, stride)).astype(f["dtype"])
            h[:, Lx:] = 0.0  # the padding: zero state, zero load, invm = 0
            x[v] = torch.from_numpy(h.reshape(-1)).to(cuda)
        ptr = lambda y, v: None if (v in ("F", "G") and not forced) else C.c_void_p(y[v].data_ptr())  # noqa: E731
        paired = {v: t.clone() for v, t in x.items()}
        N.check(getattr(N.lib, f["pair"].format(kind))(C.byref(D), *(REAL[s] for s in REAL_SCALARS[kind]), *(ptr(paired, v) for v in pointers), st), kind)
        single = {v: t.clone() for v, t in x.items()}
        for name, scalars, args in SWEEPS[kind]:
            N.check(getattr(N.lib, f["sweep"].format(name))(C.byref(D), *(REAL[s] for s in scalars), *(ptr(single, v) for v in args), st), name)
        torch.cuda.synchronize()
        for key, buf in written.items():
            a, b = paired[buf], single[key]
            where = f"{family} {kind} lattice=({nx},{ny},{nb}) stride={stride} {key}"
            assert bool(torch.isfinite(b).all()) and float(b.abs().max()) > 0 and not torch.equal(b, x[key]), where
            bad = torch.nonzero(a.view(integer) != b.view(integer)).flatten()
            assert bad.numel() == 0, f"{where}: {bad.numel()} entries differ, the first at (I, J) = ({int(bad[0]) % stride}, {int(bad[0]) // stride}): " \
                                     f"{float(a[bad[0]])!r} for {float(b[bad[0]])!r}"
            assert float(a.view(Ly, stride)[:, Lx:].abs().max() if stride > Lx else 0.0) == 0.0, where  # the padding stays zero
        for v in ALL:  # nothing else was written by the pair
            if v not in written.values():
                assert torch.equal(paired[v].view(integer), x[v].view(integer)), f"{family} {kind} ({nx},{ny},{nb}) {v}"


@pytest.mark.parametrize("family", list(FAMILIES))
def test_bad_calls_are_refused_and_write_nothing(cuda, family):
    import torch

    from cuddhelmholtz_amd import _native as N

    f = FAMILIES[family]
    nx, ny, nb = 2, 2, 4  # Lx = 7
    stride = 8
    A, w = tables(nb, seed=1)
    h = host_vectors(nx, 6, nb, 28, seed=5)  # 19 x 28 elements: room for every description tried, were one of them launched
    x = {**h, "ps2": h["ps"], "p_out": h["ps_out"], "q_out": h["ps_out"][::-1].copy()}
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = description(N, nx, ny, nb, stride, A, w)

    def attempt(kind, D=good, swap=None, off=None, absent=()):
        scalars, pointers, _, _ = KINDS[kind]
        bufs = {v: f["buf"](torch, cuda, x[v], 1 if v == off else 0) for v in pointers}
        args = [None if v in absent else bufs[(swap or {}).get(v, v)].p for v in pointers]
        err = getattr(N.lib, f["pair"].format(kind))(C.byref(D), *scalars, *args, st)
        torch.cuda.synchronize()
        assert err == 1, (kind, swap, off, absent, err)
        assert all(b.untouched() for b in bufs.values())

    # an output that is read with a halo
    for kind, swaps in (("rk2", ({"p_out": "p"}, {"q_out": "q"}, {"p_out": "q"}, {"u": "p"}, {"v": "q"})),
                        ("rk4_34", ({"p_out": "ps2"}, {"p_out": "qs"}, {"p_out": "p"}, {"u": "qs"})),
                        ("rk4_12", ({"ps2": "p"}, {"ps2": "q"}, {"qs": "q"}, {"aq": "p"}, {"ap": "q"}))):
        for swap in swaps:
            attempt(kind, swap=swap)
    for kind in KINDS:
        attempt(kind, absent=("G",))  # F without G
        attempt(kind, absent=("F",))
        attempt(kind, absent=("q" if kind != "rk4_34" else "qs",))
        attempt(kind, off="p")  # a pointer one element off a 16-byte boundary (read with a halo)
        attempt(kind, off="invm")  # ... (a stream)
        attempt(kind, off="F")
        attempt(kind, off=KINDS[kind][1][-1])  # ... (an output)
        attempt(kind, D=description(N, nx, ny, nb, 7 if family == "f64" else 10, A, w))  # a stride >= Lx of the wrong multiple
        attempt(kind, D=description(N, nx, ny, nb, 4, A, w))  # a stride below Lx = 7
        attempt(kind, D=description(N, nx, ny, 9, 28, A, w))  # n_basis beyond 8
        attempt(kind, D=description(N, 0, ny, nb, stride, A, w))
