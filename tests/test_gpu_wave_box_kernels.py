"""kernels/wave_box.hip, entry point by entry point through the C ABI, bit for bit against numpy.

The inputs are those of test_gpu_wave_lattice_kernels.py: the 1-D element matrix A holds integers in [-4, 4] and is NOT symmetric,
the weights are 1 or 2, the scale factors are the different powers of two cx = 2, cy = 1/2, cz = 4 (a swapped axis shows), every
vector holds small integers, invm and every coefficient are powers of two.  The stencil and each stage are then exact in float64
whatever the order of their operations (asserted on the CPU: the float64 chain equals the chain summed backwards in longdouble),
and the kernels are held to the numpy restatement of include/cuddh_hip.h bit for bit.  The restatement is written from the
header, line by line (`line` of the 2-D file: which element rows a node of a line reads), not from the kernel's tables.

Lattices (nx, ny, nz, n_basis), the smallest at which each path changes: (1,1,1,2); (3,1,1,4), (1,3,1,4), (1,1,3,4): one element
in two directions; (2,2,2,3), (2,1,2,5), (1,2,2,6), (2,1,1,8) on the run-time n_basis instantiation.  A workgroup's tile is
TX x TY x TZ nodes (cuddh_hip_wave_box_tile_x / _y / _z, read from the library): with n_basis 2 (L = n + 1) every direction gets
lattices of tile - 1, tile and tile + 1 nodes (at least 2, the smallest line there is).  A kernel that walks element layers in z
(TZ > 1) also gets a lattice whose z run ends inside a walk and one that needs two walks; with TZ = 1 a workgroup owns one plane
and there is no walk.  (43, 6, 2, 4) has 2 x 2 x 7 = 28 workgroups, more than the eight slots the ids are dealt over and no
multiple of eight.  Lx is odd (a padding column) in (2,2,2,3), (2,1,2,5), (2,1,1,8) and even in the n_basis 4 lattices here.

Both the forced form (F, G given) and the homogeneous form (both NULL).  Every buffer has 16 elements of a NaN pattern on both
sides; after each call the guards, and every vector the stage does not write, are compared bitwise with what they held.  Every
refusal returns 1 and writes nothing; the same call twice gives the same bits.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_wave_lattice_kernels import STAGES, VECTORS, line, tables
from test_gpu_wave_stage_kernels import CS, DT, FILT, HALF_DT, SN, Buf

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

CX, CY, CZ = 2.0, 0.5, 4.0
FIXED = [(1, 1, 1, 2), (3, 1, 1, 4), (1, 3, 1, 4), (1, 1, 3, 4), (2, 2, 2, 3), (2, 1, 2, 5), (1, 2, 2, 6), (2, 1, 1, 8), (43, 6, 2, 4)]


def tile():
    from cuddhelmholtz_amd import _native as N

    return N.lib.cuddh_hip_wave_box_tile_x(), N.lib.cuddh_hip_wave_box_tile_y(), N.lib.cuddh_hip_wave_box_tile_z()


@functools.lru_cache(maxsize=None)
def lattices():
    """FIXED and the lattices around the tile sizes"""
    out = list(FIXED)
    for axis, T in enumerate(tile()):
        for L in sorted({max(2, T - 1), max(2, T), T + 1}):  # nodes; n_basis 2 has L = n + 1
            n = [1, 1, 1]
            n[axis] = L - 1
            out.append((*n, 2))
    TZ = tile()[2]
    if TZ > 1:  # a z run that ends inside a walk, and two walks (n_basis 3: an element layer is two planes)
        out += [(1, 1, max(1, (TZ + TZ // 2) // 2), 3), (1, 1, TZ + 1, 3)]
    return tuple(dict.fromkeys(out))


def dims(nx, ny, nz, nb):
    H = nb - 1
    Lx = nx * H + 1
    return Lx, ny * H + 1, nz * H + 1, Lx + Lx % 2


def stencil(nx, ny, nz, nb, A, w, p, dtype=np.float64, backwards=False):
    """K p on the padded lattice vector p (stride * Ly * Lz) as include/cuddh_hip.h states it; zero in the padding columns"""
    Lx, Ly, Lz, stride = dims(nx, ny, nz, nb)
    P = p.reshape(Lz, Ly, stride).astype(dtype)
    sx, sy, sz = (np.zeros((Lz, Ly, stride), dtype=dtype) for _ in range(3))
    lx, ly, lz = line(nx, nb, A, w), line(ny, nb, A, w), line(nz, nb, A, w)
    order = (lambda t: list(t)[::-1]) if backwards else list
    for I, (terms, _) in enumerate(lx):
        for d, c in order(terms):
            assert 0 <= I + d < Lx
            sx[:, :, I] += dtype(c) * P[:, :, I + d]
    for J, (terms, _) in enumerate(ly):
        for d, c in order(terms):
            assert 0 <= J + d < Ly
            sy[:, J, :Lx] += dtype(c) * P[:, J + d, :Lx]
    for K, (terms, _) in enumerate(lz):
        for d, c in order(terms):
            assert 0 <= K + d < Lz
            sz[K, :, :Lx] += dtype(c) * P[K + d, :, :Lx]
    Wx = np.zeros(stride, dtype=dtype)
    Wx[:Lx] = [wt for _, wt in lx]
    Wy, Wz = np.array([wt for _, wt in ly], dtype=dtype), np.array([wt for _, wt in lz], dtype=dtype)
    ax = dtype(CX) * (Wy[None, :, None] * Wz[:, None, None])
    ay = dtype(CY) * (Wx[None, None, :] * Wz[:, None, None])
    az = dtype(CZ) * (Wx[None, None, :] * Wy[None, :, None])
    Kp = (az * sz + ay * sy) + ax * sx if backwards else ax * sx + (ay * sy + az * sz)
    Kp[:, :, Lx:] = 0
    return Kp.reshape(-1)


def host_vectors(nx, ny, nz, nb, seed):
    Lx, Ly, Lz, stride = dims(nx, ny, nz, nb)
    rng = np.random.default_rng(seed)
    x = {name: rng.integers(-8, 9, (Lz, Ly, stride)).astype(np.float64) for name in VECTORS}
    x["invm"] = 2.0 ** rng.integers(-1, 2, (Lz, Ly, stride))
    x["Hi"] = rng.integers(0, 3, (Lz, Ly, stride)).astype(np.float64)
    for v in x.values():
        v[:, :, Lx:] = 0.0  # the padding: zero state, zero load, invm = 0
    return {name: v.reshape(-1) for name, v in x.items()}


def description(N, nx, ny, nz, nb, stride, A, w):
    D = N.WaveBox()
    D.nx, D.ny, D.nz, D.n_basis, D.stride, D.cx, D.cy, D.cz = nx, ny, nz, nb, stride, CX, CY, CZ
    for i, a in enumerate(A.reshape(-1)):
        D.A[i] = a
    for i, a in enumerate(w):
        D.w[i] = a
    return D


def seed_of(nx, ny, nz, nb):
    return 100000 * nx + 1000 * ny + 10 * nz + nb


def test_every_box_entry_point_is_covered_and_the_chain_is_exact():
    from cuddhelmholtz_amd import _native as N

    declared = {s for s in N.declared_symbols() if s.startswith("cuddh_hip_wave_box_")}
    assert declared == {f"cuddh_hip_wave_box_{name}_f64" for name in STAGES} | {f"cuddh_hip_wave_box_tile_{a}" for a in "xyz"}
    TX, TY, TZ = tile()
    assert TX >= 2 and TY >= 1 and TZ >= 1
    found = lattices()
    assert {dims(*lat)[0] % 2 for lat in found} == {0, 1}  # odd and even Lx
    for axis, T in enumerate((TX, TY, TZ)):
        assert {max(2, T - 1), max(2, T), T + 1} <= {dims(*lat)[axis] for lat in found if lat[3] == 2}
    # float64 forwards equals longdouble backwards: every partial sum of the chain is exact on these inputs
    for lat in found:
        A, w = tables(lat[3], seed=lat[3])
        x = host_vectors(*lat, seed=seed_of(*lat))
        for v in ("p", "ps"):
            forwards = stencil(*lat, A, w, x[v])
            assert np.array_equal(forwards.astype(np.longdouble), stencil(*lat, A, w, x[v], dtype=np.longdouble, backwards=True)), lat
            assert np.any(forwards != 0)


@pytest.mark.parametrize("name,forced", [(name, forced) for name in STAGES for forced in (True, False)],
                         ids=lambda v: v if isinstance(v, str) else ("forced" if v else "homogeneous"))
def test_box_stage_matches_numpy_bit_for_bit(cuda, name, forced):
    import torch

    from cuddhelmholtz_amd import _native as N

    scalars, stencil_input, pointers, written, ref = STAGES[name]
    fn = getattr(N.lib, f"cuddh_hip_wave_box_{name}_f64")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for lat in lattices():
        nx, ny, nz, nb = lat
        Lx, Ly, Lz, stride = dims(*lat)
        A, w = tables(nb, seed=nb)
        x = host_vectors(*lat, seed=seed_of(*lat))
        x["w"] = stencil(*lat, A, w, x[stencil_input])
        want = ref(x, forced)
        bufs = {v: Buf(torch, cuda, x[v], 0) for v in pointers}
        args = [None if (v in ("F", "G") and not forced) else bufs[v].p for v in pointers]
        D = description(N, *lat, stride, A, w)
        N.check(fn(C.byref(D), *scalars, *args, st), name)
        torch.cuda.synchronize()
        target = {buf: key for key, buf in written.items()}
        first = {v: bufs[v].bits().copy() for v in pointers}
        for v in pointers:
            where = f"{name} lattice={lat} {v}"
            if v in target:
                got = bufs[v].get()
                expected = np.ascontiguousarray(want[target[v]])
                bad = np.flatnonzero(got.view(np.uint64) != expected.view(np.uint64))
                assert bad.size == 0, f"{where}: {bad.size} entries differ, the first at (I, J, K) = ({bad[0] % stride}, " \
                                      f"{bad[0] // stride % Ly}, {bad[0] // (stride * Ly)}): {got[bad[0]]} for {expected[bad[0]]}"
            else:
                assert bufs[v].untouched(), where
        if lat in ((2, 2, 2, 3), (43, 6, 2, 4)):  # the same call on the same inputs again: the same bits
            again = {v: Buf(torch, cuda, x[v], 0) for v in pointers}
            args = [None if (v in ("F", "G") and not forced) else again[v].p for v in pointers]
            N.check(fn(C.byref(D), *scalars, *args, st), name)
            torch.cuda.synchronize()
            for v in pointers:
                assert np.array_equal(again[v].bits(), first[v]), f"{name} lattice={lat} {v}: a second call gave other bits"


def test_forced_form_with_zero_load_gives_the_homogeneous_bits_and_calls_repeat(cuda):
    """on non-integer data, where rounding happens: compile-time and run-time n_basis"""
    import torch

    from cuddhelmholtz_amd import _native as N

    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for lat in ((5, 3, 4, 4), (3, 2, 3, 5)):
        nb = lat[3]
        Lx, Ly, Lz, stride = dims(*lat)
        rng = np.random.default_rng(3)
        A, w = rng.standard_normal((nb, nb)), rng.random(nb) + 0.5
        D = description(N, *lat, stride, A, w)
        D.cx, D.cy, D.cz = 0.7, 1.3, 2.1
        pad = np.ones((Lz, Ly, stride))
        pad[:, :, Lx:] = 0.0
        x = {v: torch.from_numpy((rng.standard_normal((Lz, Ly, stride)) * pad).reshape(-1)).to(cuda) for v in ("ps", "p", "q", "invm", "Hi", "qs", "aq", "ap")}
        outs = []
        for forced in (False, True, True):
            y = {v: t.clone() for v, t in x.items()}
            y["ps_out"] = torch.zeros_like(x["ps"])
            zero = torch.zeros_like(x["ps"])
            fg = [C.c_void_p(zero.data_ptr())] * 2 if forced else [None, None]
            ptr = lambda v: C.c_void_p(y[v].data_ptr())  # noqa: E731
            N.check(N.lib.cuddh_hip_wave_box_rk4_2_f64(C.byref(D), 0.37, 0.8, -0.6, ptr("ps"), ptr("p"), ptr("q"), ptr("invm"), ptr("Hi"), *fg,
                                                       ptr("ps_out"), ptr("qs"), ptr("aq"), ptr("ap"), st), "rk4_2")
            torch.cuda.synchronize()
            outs.append(y)
        for v in ("ps_out", "qs", "aq", "ap"):
            assert torch.equal(outs[0][v], outs[1][v]) and torch.equal(outs[1][v], outs[2][v]) and bool(torch.isfinite(outs[0][v]).all()), (lat, v)
        assert float(outs[0]["ps_out"].abs().max()) > 0 and not torch.equal(outs[0]["qs"], x["qs"])
        # the padding columns stay zero
        assert float(outs[0]["qs"].reshape(Lz, Ly, stride)[:, :, Lx:].abs().max() if stride > Lx else 0.0) == 0.0


def test_bad_calls_are_refused_and_write_nothing(cuda):
    import torch

    from cuddhelmholtz_amd import _native as N

    lat = (2, 2, 2, 4)
    nb = 4
    stride = 8
    A, w = tables(nb, seed=1)
    x = host_vectors(*lat, seed=5)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pointers = STAGES["rk4_2"][2]

    def attempt(D, swap=None, off=None, null=None):
        bufs = {v: Buf(torch, cuda, x[v], 1 if v == off else 0) for v in pointers}
        args = [None if v == null else bufs[(swap or {}).get(v, v)].p for v in pointers]
        err = N.lib.cuddh_hip_wave_box_rk4_2_f64(None if D is None else C.byref(D), HALF_DT, CS, SN, *args, st)
        torch.cuda.synchronize()
        assert err == 1, (swap, off, null, err)
        assert all(b.untouched() for b in bufs.values())

    good = description(N, *lat, stride, A, w)
    attempt(good, swap={"ps_out": "ps"})  # ps_in == ps_out
    attempt(good, off="q")  # a pointer that is not 16-byte aligned
    attempt(good, null="qs")  # a NULL vector
    attempt(good, null="G")  # F without G
    attempt(good, null="F")
    attempt(None)  # no description
    attempt(description(N, 2, 2, 2, nb, 7, A, w))  # an odd stride
    attempt(description(N, 2, 2, 2, nb, 6, A, w))  # a stride below Lx = 7
    attempt(description(N, 2, 2, 2, 9, 20, A, w))  # n_basis beyond 8
    attempt(description(N, 2, 2, 2, 1, stride, A, w))  # and below 2
    for bad in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (2, 2, -1)):
        attempt(description(N, *bad, nb, stride, A, w))
    attempt(description(N, 2, 40000, 40000, nb, stride, A, w))  # stride Ly Lz beyond an int
    # rk2_b writes p, q, u, v: its stencil input cannot be one of them
    bufs = {v: Buf(torch, cuda, x[v], 0) for v in STAGES["rk2_b"][2]}
    args = [bufs["p" if v == "ps" else v].p for v in STAGES["rk2_b"][2]]
    assert N.lib.cuddh_hip_wave_box_rk2_b_f64(C.byref(good), DT, CS, SN, FILT, *args, st) == 1
    torch.cuda.synchronize()
    assert all(b.untouched() for b in bufs.values())
