"""kernels/wave_lattice.hip, entry point by entry point through the C ABI, bit for bit against numpy.

The 1-D element matrix A holds integers in [-4, 4] and is NOT symmetric (a transposed index shows), the weights are 1 or 2, the
scale factors are the different powers of two cx = 2, cy = 1/2 (a swapped x / y shows), every vector holds small integers, invm
is a power of two and every coefficient too: the stencil and each stage are exact in float64 whatever the order of their
operations, and the kernels are held to the numpy restatement of include/cuddh_hip.h bit for bit.  The restatement is written from
the header's description node by node (which element rows a node reads), not from the kernel's tables.

Lattices (nx, ny, n_basis), the smallest at which each path changes: (1,1,2); (1,3,4) and (3,1,4), one element in a direction;
(2,2,3); (3,2,5); (2,3,6) and (3,2,8) on the run-time n_basis instantiation.  A tile of the kernel is TX x TY = 128 x 16 nodes
(cuddh_hip_wave_lattice_tile_x / _y, read from the library here).  n_basis 4 has Lx = 3 nx + 1, so around TX it takes 124, 127
and 130 (nx = 41, 42, 43): 124 leaves columns of the tile idle, 127 with its padding column is a row of exactly 128 doubles, one
tile, and 130 spills two nodes into a second tile; Ly = 13, 16, 19 (ny = 4, 5, 6) is one less row-block, exactly a tile and one
more.  Lx = TX - 1, TX, TX + 1 exactly with n_basis 2 (nx = 126, 127, 128), and Lx = TX + 1 with n_basis 5 (nx = 32).
(43, 27, 4) has 12 tiles, more than the eight the workgroup ids are dealt over and no multiple of it.  Lx is odd (a padding
column: zero state, invm = 0, never read by the stencil, kept zero) in most of these and even in (41, *, 4), (43, *, 4),
(127, 1, 2) and (1, 1, 2).

Both the forced form (F, G given) and the homogeneous form (both NULL).  Every buffer has 16 elements of a NaN pattern on both
sides; after each call the guards, and every vector the stage does not write, are compared bitwise with what they held.
rk4_2 / rk4_3 with ps_in == ps_out, a stencil input among the outputs, an odd stride and a misaligned pointer return an error and
write nothing.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_wave_stage_kernels import CS, DT, FILT, HALF_DT, SIXTH_DT, SN, Buf, ref_rk2_a, ref_rk2_b, ref_rk4_1, ref_rk4_4, ref_rk4_mid

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

CX, CY = 2.0, 0.5
LATTICES = [(1, 1, 2), (1, 3, 4), (3, 1, 4), (2, 2, 3), (3, 2, 5), (2, 3, 6), (3, 2, 8),
            (41, 4, 4), (42, 5, 4), (43, 6, 4), (42, 4, 4), (41, 6, 4), (43, 27, 4),
            (126, 1, 2), (127, 1, 2), (128, 2, 2), (32, 1, 5)]

# name -> (leading scalars, the stencil's input, pointer arguments in the entry point's order, {reference name: buffer written}, numpy restatement)
STAGES = {
    "rk2_a": ((HALF_DT, CS, SN), "p", ("p", "q", "invm", "Hi", "F", "G", "qs", "ps"), {"qs": "qs", "ps": "ps"}, ref_rk2_a),
    "rk2_b": ((DT, CS, SN, FILT), "ps", ("ps", "qs", "invm", "Hi", "F", "G", "p", "q", "u", "v"), {v: v for v in "pquv"}, ref_rk2_b),
    "rk4_1": ((HALF_DT, CS, SN), "p", ("p", "q", "invm", "Hi", "F", "G", "ps", "qs", "aq", "ap"), {v: v for v in ("ps", "qs", "aq", "ap")}, ref_rk4_1),
    "rk4_2": ((HALF_DT, CS, SN), "ps", ("ps", "p", "q", "invm", "Hi", "F", "G", "ps_out", "qs", "aq", "ap"),
              {"ps": "ps_out", "qs": "qs", "aq": "aq", "ap": "ap"}, ref_rk4_mid(HALF_DT)),
    "rk4_3": ((DT, CS, SN), "ps", ("ps", "p", "q", "invm", "Hi", "F", "G", "ps_out", "qs", "aq", "ap"),
              {"ps": "ps_out", "qs": "qs", "aq": "aq", "ap": "ap"}, ref_rk4_mid(DT)),
    "rk4_4": ((SIXTH_DT, CS, SN, FILT), "ps", ("ps", "qs", "aq", "ap", "invm", "Hi", "F", "G", "p", "q", "u", "v"), {v: v for v in "pquv"}, ref_rk4_4),
}
VECTORS = ("p", "q", "u", "v", "ps", "ps_out", "qs", "aq", "ap", "F", "G", "invm", "Hi")


def tables(nb, seed):
    rng = np.random.default_rng(seed)
    A = rng.integers(-4, 5, (nb, nb)).astype(np.float64)
    A[0, nb - 1], A[nb - 1, 0] = 3.0, -2.0  # not symmetric, whatever was drawn
    w = rng.integers(1, 3, nb).astype(np.float64)
    return A, w


def line(n, nb, A, w):
    """per node of a line of n elements: ([(offset, coefficient)], weight), from the element rows the node reads"""
    H = nb - 1
    L = n * H + 1
    out = []
    for i in range(L):
        k = i % H
        if k:  # interior of element i // H: row k
            out.append(([(j - k, A[k, j]) for j in range(nb)], w[k]))
            continue
        terms, weight = {}, 0.0
        if i > 0:  # last row of the element to the left
            for j in range(nb):
                terms[j - H] = terms.get(j - H, 0.0) + A[H, j]
            weight += w[H]
        if i < L - 1:  # first row of the element to the right
            for j in range(nb):
                terms[j] = terms.get(j, 0.0) + A[0, j]
            weight += w[0]
        out.append((sorted(terms.items()), weight))
    return out


def stencil(nx, ny, nb, stride, A, w, p):
    """K p on the padded lattice vector p (stride * Ly): zero in the padding columns"""
    H = nb - 1
    Lx, Ly = nx * H + 1, ny * H + 1
    P = p.reshape(Ly, stride)
    sx, sy = np.zeros((Ly, stride)), np.zeros((Ly, stride))
    lx, ly = line(nx, nb, A, w), line(ny, nb, A, w)
    for I, (terms, _) in enumerate(lx):
        for d, c in terms:
            assert 0 <= I + d < Lx
            sx[:, I] += c * P[:, I + d]
    for J, (terms, _) in enumerate(ly):
        for d, c in terms:
            assert 0 <= J + d < Ly
            sy[J, :Lx] += c * P[J + d, :Lx]
    Wx, Wy = np.zeros(stride), np.array([wt for _, wt in ly])
    Wx[:Lx] = [wt for _, wt in lx]
    K = (CX * Wy)[:, None] * sx + (CY * Wx)[None, :] * sy
    K[:, Lx:] = 0.0
    return K.reshape(-1)


def host_vectors(nx, ny, nb, stride, seed):
    H = nb - 1
    Lx, Ly = nx * H + 1, ny * H + 1
    rng = np.random.default_rng(seed)
    x = {name: rng.integers(-8, 9, (Ly, stride)).astype(np.float64) for name in VECTORS}
    x["invm"] = 2.0 ** rng.integers(-1, 2, (Ly, stride))
    x["Hi"] = rng.integers(0, 3, (Ly, stride)).astype(np.float64)
    for v in x.values():
        v[:, Lx:] = 0.0  # the padding: zero state, zero load, invm = 0
    return {name: v.reshape(-1) for name, v in x.items()}


def description(N, nx, ny, nb, stride, A, w):
    D = N.WaveLattice()
    D.nx, D.ny, D.n_basis, D.stride, D.cx, D.cy = nx, ny, nb, stride, CX, CY
    for i, a in enumerate(A.reshape(-1)):
        D.A[i] = a
    for i, a in enumerate(w):
        D.w[i] = a
    return D


def test_every_lattice_entry_point_is_covered():
    from cuddhelmholtz_amd import _native as N

    declared = {s for s in N.declared_symbols() if s.startswith("cuddh_hip_wave_lattice_")}
    assert declared == {f"cuddh_hip_wave_lattice_{name}_f64" for name in (*STAGES, "begin", "gather")} | {"cuddh_hip_wave_lattice_tile_x",
                                                                                                           "cuddh_hip_wave_lattice_tile_y"}
    assert (N.lib.cuddh_hip_wave_lattice_tile_x(), N.lib.cuddh_hip_wave_lattice_tile_y()) == (128, 16)  # what LATTICES is built around


@pytest.mark.parametrize("name,forced", [(name, forced) for name in STAGES for forced in (True, False)],
                         ids=lambda v: v if isinstance(v, str) else ("forced" if v else "homogeneous"))
def test_lattice_stage_matches_numpy_bit_for_bit(cuda, name, forced):
    import torch

    from cuddhelmholtz_amd import _native as N

    scalars, stencil_input, pointers, written, ref = STAGES[name]
    fn = getattr(N.lib, f"cuddh_hip_wave_lattice_{name}_f64")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for nx, ny, nb in LATTICES:
        Lx = nx * (nb - 1) + 1
        stride = Lx + Lx % 2
        A, w = tables(nb, seed=nb)
        x = host_vectors(nx, ny, nb, stride, seed=1000 * nx + 10 * ny + nb)
        x["w"] = stencil(nx, ny, nb, stride, A, w, x[stencil_input])
        want = ref(x, forced)
        bufs = {v: Buf(torch, cuda, x[v], 0) for v in pointers}
        args = [None if (v in ("F", "G") and not forced) else bufs[v].p for v in pointers]
        D = description(N, nx, ny, nb, stride, A, w)
        N.check(fn(C.byref(D), *scalars, *args, st), name)
        torch.cuda.synchronize()
        target = {buf: key for key, buf in written.items()}
        for v in pointers:
            where = f"{name} lattice=({nx},{ny},{nb}) {v}"
            if v in target:
                got = bufs[v].get()
                expected = np.ascontiguousarray(want[target[v]])
                bad = np.flatnonzero(got.view(np.uint64) != expected.view(np.uint64))
                assert bad.size == 0, f"{where}: {bad.size} entries differ, the first at (I, J) = ({bad[0] % stride}, {bad[0] // stride}): " \
                                      f"{got[bad[0]]} for {expected[bad[0]]}"
            else:
                assert bufs[v].untouched(), where


def test_forced_form_with_zero_load_gives_the_homogeneous_bits(cuda):
    """on non-integer data, where rounding happens"""
    import torch

    from cuddhelmholtz_amd import _native as N

    nx, ny, nb = 5, 7, 4
    Lx, Ly = nx * 3 + 1, ny * 3 + 1
    rng = np.random.default_rng(3)
    A, w = rng.standard_normal((nb, nb)), rng.random(nb) + 0.5
    D = description(N, nx, ny, nb, Lx, A, w)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = {v: torch.from_numpy(rng.standard_normal(Lx * Ly)).to(cuda) for v in ("ps", "p", "q", "invm", "Hi", "qs", "aq", "ap")}
    outs = []
    for forced in (False, True):
        y = {v: t.clone() for v, t in x.items()}
        y["ps_out"] = torch.zeros_like(x["ps"])
        zero = torch.zeros_like(x["ps"])
        fg = [C.c_void_p(zero.data_ptr())] * 2 if forced else [None, None]
        ptr = lambda v: C.c_void_p(y[v].data_ptr())  # noqa: E731
        N.check(N.lib.cuddh_hip_wave_lattice_rk4_2_f64(C.byref(D), 0.37, 0.8, -0.6, ptr("ps"), ptr("p"), ptr("q"), ptr("invm"), ptr("Hi"), *fg,
                                                       ptr("ps_out"), ptr("qs"), ptr("aq"), ptr("ap"), st), "rk4_2")
        torch.cuda.synchronize()
        outs.append(y)
    for v in ("ps_out", "qs", "aq", "ap"):
        assert torch.equal(outs[0][v], outs[1][v]) and bool(torch.isfinite(outs[0][v]).all()), v
    assert float(outs[0]["ps_out"].abs().max()) > 0 and not torch.equal(outs[0]["qs"], x["qs"])


def test_bad_calls_are_refused_and_write_nothing(cuda):
    import torch

    from cuddhelmholtz_amd import _native as N

    nx, ny, nb = 2, 2, 4
    stride = 8
    A, w = tables(nb, seed=1)
    x = host_vectors(nx, ny, nb, stride, seed=5)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pointers = STAGES["rk4_2"][2]

    def attempt(D, swap=None, off=None):
        bufs = {v: Buf(torch, cuda, x[v], 1 if v == off else 0) for v in pointers}
        args = [bufs[(swap or {}).get(v, v)].p for v in pointers]
        err = N.lib.cuddh_hip_wave_lattice_rk4_2_f64(C.byref(D), HALF_DT, CS, SN, *args, st)
        torch.cuda.synchronize()
        assert err == 1, (swap, off, err)
        assert all(b.untouched() for b in bufs.values())

    good = description(N, nx, ny, nb, stride, A, w)
    attempt(good, swap={"ps_out": "ps"})  # ps_in == ps_out
    attempt(good, off="q")  # a pointer that is not 16-byte aligned
    attempt(description(N, nx, ny, nb, 7, A, w))  # an odd stride
    attempt(description(N, nx, ny, nb, 6, A, w))  # a stride below Lx = 7
    attempt(description(N, nx, ny, 9, 20, A, w))  # n_basis beyond 8
    attempt(description(N, 0, ny, nb, stride, A, w))
    # rk2_b writes p, q, u, v: its stencil input cannot be one of them
    bufs = {v: Buf(torch, cuda, x[v], 0) for v in STAGES["rk2_b"][2]}
    args = [bufs["p" if v == "ps" else v].p for v in STAGES["rk2_b"][2]]
    assert N.lib.cuddh_hip_wave_lattice_rk2_b_f64(C.byref(good), DT, CS, SN, FILT, *args, st) == 1
    torch.cuda.synchronize()
    assert all(b.untouched() for b in bufs.values())


def test_gather_and_begin_bit_for_bit(cuda):
    import torch

    from cuddhelmholtz_amd import _native as N

    rng = np.random.default_rng(9)
    ndof, n = 1500, 1620
    slot_of = rng.permutation(n)[:ndof]
    dof_of = np.full(n, -1, dtype=np.int32)
    dof_of[slot_of] = np.arange(ndof, dtype=np.int32)
    zu, zv = rng.standard_normal(ndof), rng.standard_normal(ndof)
    lat = lambda z: np.where(dof_of >= 0, z[np.maximum(dof_of, 0)], 0.0)  # noqa: E731
    d_dof = torch.from_numpy(dof_of).to(cuda)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bufs = {"zu": Buf(torch, cuda, zu, 0), "zv": Buf(torch, cuda, zv, 1)}
    out = {v: Buf(torch, cuda, np.full(n, 7.0), 0) for v in "pquvy"}
    N.check(N.lib.cuddh_hip_wave_lattice_begin_f64(n, FILT, C.c_void_p(d_dof.data_ptr()), bufs["zu"].p, bufs["zv"].p, out["p"].p, out["q"].p, out["u"].p,
                                                   out["v"].p, st), "begin")
    N.check(N.lib.cuddh_hip_wave_lattice_gather_f64(n, C.c_void_p(d_dof.data_ptr()), bufs["zv"].p, out["y"].p, st), "gather")
    torch.cuda.synchronize()
    for v, want in (("p", lat(zu)), ("q", lat(zv)), ("u", FILT * lat(zu)), ("v", FILT * lat(zv)), ("y", lat(zv))):
        assert np.array_equal(out[v].get().view(np.uint64), want.view(np.uint64)), v
    assert bufs["zu"].untouched() and bufs["zv"].untouched()
