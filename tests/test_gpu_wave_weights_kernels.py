"""kernels/wave_weights.hip and wave_weights_f32.hip (lattice sweeps with a per-cell stiffness weight), entry point by entry point
through the C ABI.

(a) Bit for bit against numpy.  The data is that of test_gpu_wave_cells_kernels.py (integer, non-symmetric tables, weights of the
rule 1 or 2, cx = 2, cy = 1/2, small integer vectors, powers of two elsewhere) and the cell weights are integers in {0, 1, 2, 3}.
The restatement is not the kernel's regrouping per node but what that regroups, the sum over the cells of beta_e times the
element's own Kronecker sum
    (K_e p)[b, a] = cx w[b] sum_a' A[a][a'] p[b, a'] + cy w[a] sum_b' A[b][b'] p[b', a]        on the cell's n_basis x n_basis nodes.
That the chain (stencil, then stage) is exact is asserted on the CPU first: the float64 run equals a longdouble run that adds the
cells up backwards, and for the fp32 family a float32 run equals it too.  Weight patterns: all ones; all threes; random in
{0, 1, 2, 3}; one non-zero cell; a jump (1 | 3, 2 above) at the cell column and row that begin at the tile boundary where H
divides 128 and 16 (the jump is on it) and contain it elsewhere (a cell of the other weight reaches across it), and the same
jump one cell earlier; only the cells of tile (0, 0) non-zero (three all-zero tiles beside a full one); zeros on the lattice boundary.
A workgroup whose tile of 128 x 16 nodes has no node in a cell of non-zero weight writes nothing: every output keeps its bits.

(b) Bit for bit against the wave_cells launches: standard_normal vectors, real tables, non-dyadic scalars, the weights the flags of
that file's eight patterns as reals.  No tolerance: the gate on the order of operations.

(c) Bad calls return hipErrorInvalidValue (1) and write nothing.

The seven lattices are those of test_gpu_wave_cells_kernels.py: the smallest at which tile edges, odd Lx, cell edges on tile
boundaries and every run-time n_basis class occur.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_wave_cells_kernels import LATTICES, PATTERNS, TX, TY, flags, stride_of, void_nodes, written
from test_gpu_wave_lattice_f32_kernels import Buf32, exact32
from test_gpu_wave_lattice_kernels import CX, CY, STAGES, description, host_vectors, tables
from test_gpu_wave_stage_kernels import CS, DT, FILT, HALF_DT, SN, Buf

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

WEIGHTS = ("ones", "threes", "random", "one", "jump-on", "jump-across", "first-tile", "boundary")
FAMILY = {False: "cuddh_hip_wave_weights_%s_f64", True: "cuddh_hip_wave_weights32_%s"}
CELLS = {False: "cuddh_hip_wave_cells_%s_f64", True: "cuddh_hip_wave_cells32_%s"}


@functools.lru_cache(maxsize=None)
def weights(nx, ny, nb, pattern):
    """(ny, nx) float64 integers in {0, 1, 2, 3}, read-only"""
    H = nb - 1
    aE, bE = TX // H, TY // H  # the cell column / row that begins at the tile boundary (H divides it) or contains it
    b = np.ones((ny, nx))
    if pattern == "threes":
        b[:] = 3.0
    elif pattern == "random":
        b[:] = np.random.default_rng(7 * nx + ny).integers(0, 4, (ny, nx))
    elif pattern == "one":
        b[:] = 0.0
        b[ny // 2, nx // 2] = 2.0
    elif pattern in ("jump-on", "jump-across"):
        s = 0 if pattern == "jump-on" else 1
        b[:, max(min(aE, nx - 1) - s, 1):] = 3.0
        b[max(min(bE, ny - 1) - s, 1):, :] = 2.0
    elif pattern == "first-tile":
        b[:] = 0.0
        b[: max(1, (TY - 1) // H), : max(1, (TX - 1) // H)] = 3.0
    elif pattern == "boundary":
        b[:] = 2.0
        b[0, :] = 0.0
        b[:, nx - 1] = 0.0
        b[ny - 1, 0] = 0.0
    if not b.any():
        b[0, 0] = 1.0
    b.setflags(write=False)
    return b


def stencil_weights(nx, ny, nb, stride, A, w, beta, p, dtype=np.float64, reverse=False):
    """K p on the padded lattice vector p: the sum over the cells of beta_e times the element matrix, in `dtype`, the cells in
    ascending (reverse: descending) order"""
    H = nb - 1
    Ly = ny * H + 1
    A, w, beta = A.astype(dtype), w.astype(dtype), beta.astype(dtype)
    cx, cy = dtype(CX), dtype(CY)
    P, K = p.astype(dtype).reshape(Ly, stride), np.zeros((Ly, stride), dtype=dtype)
    cells = [(b, a) for b in range(ny) for a in range(nx) if beta[b, a] != 0]
    for b, a in (reversed(cells) if reverse else cells):
        sl = (slice(b * H, b * H + nb), slice(a * H, a * H + nb))
        loc = P[sl]
        sx = sum((A[:, k][None, :] * loc[:, k][:, None] for k in (range(nb - 1, -1, -1) if reverse else range(nb))), np.zeros((nb, nb), dtype=dtype))
        sy = sum((A[:, k][:, None] * loc[k, :][None, :] for k in (range(nb - 1, -1, -1) if reverse else range(nb))), np.zeros((nb, nb), dtype=dtype))
        K[sl] += beta[b, a] * (cx * w[:, None] * sx + cy * w[None, :] * sy)
    return K.reshape(-1)


@functools.lru_cache(maxsize=None)
def case(nx, ny, nb, pattern, stencil_input, f32):
    """(A, w, weights, vectors with the stencil of `stencil_input` as "w", written slots), computed once and never changed"""
    stride = stride_of(nx, nb, f32)
    A, w = tables(nb, seed=nb)
    beta = weights(nx, ny, nb, pattern)
    x = host_vectors(nx, ny, nb, stride, seed=1000 * nx + 10 * ny + nb)
    void = void_nodes(nx, ny, nb, stride, beta != 0)
    x["invm"] = np.where(void, 0.0, x["invm"])
    x["w"] = stencil_weights(nx, ny, nb, stride, A, w, beta, x[stencil_input])
    assert not x["w"][void].any()
    for v in x.values():
        v.setflags(write=False)
    return A, w, beta, x, written(nx, ny, nb, stride, beta != 0)


def chain(nx, ny, nb, pattern, name, forced, dtype, reverse):
    """stencil and stage of one case in `dtype`: {reference name: vector}"""
    _, stencil_input, _, _, ref = STAGES[name]
    A, w, beta, x, _ = case(nx, ny, nb, pattern, stencil_input, False)
    y = {k: v.astype(dtype) for k, v in x.items()}
    y["w"] = stencil_weights(nx, ny, nb, stride_of(nx, nb, False), A, w, beta, x[stencil_input], dtype=dtype, reverse=reverse)
    return ref(y, forced)


def test_the_chain_is_exact_and_the_patterns_are_what_the_docstring_says():
    """(no device) float64 forwards = longdouble backwards = float32, for every stage on the lattices with the largest sums; the
    restatement at 0 / 1 weights is test_gpu_wave_cells_kernels' one"""
    from test_gpu_wave_cells_kernels import stencil_cells

    for nx, ny, nb in ((3, 2, 8), (2, 3, 6), (33, 5, 5)):
        for pattern in ("threes", "random", "jump-on"):
            for name in STAGES:
                for forced in (True, False):
                    f64 = chain(nx, ny, nb, pattern, name, forced, np.float64, False)
                    ld = chain(nx, ny, nb, pattern, name, forced, np.longdouble, True)
                    f32 = chain(nx, ny, nb, pattern, name, forced, np.float32, False)
                    for k in f64:
                        assert f64[k].dtype == np.float64 and ld[k].dtype == np.longdouble and f32[k].dtype == np.float32
                        assert np.array_equal(f64[k].astype(np.longdouble), ld[k]), (nx, ny, nb, pattern, name, forced, k)
                        assert np.array_equal(f32[k].astype(np.float64), f64[k]), (nx, ny, nb, pattern, name, forced, k)
    for nx, ny, nb in LATTICES:
        stride = stride_of(nx, nb, False)
        A, w = tables(nb, seed=nb)
        p = host_vectors(nx, ny, nb, stride, seed=3)["p"]
        for pattern in ("random", "edge"):
            f = flags(nx, ny, nb, pattern)
            assert np.array_equal(stencil_weights(nx, ny, nb, stride, A, w, f.astype(np.float64), p), stencil_cells(nx, ny, nb, stride, A, w, f, p))
        assert np.array_equal(stencil_weights(nx, ny, nb, stride, A, w, weights(nx, ny, nb, "threes"), p),
                              3.0 * stencil_weights(nx, ny, nb, stride, A, w, weights(nx, ny, nb, "ones"), p))
        for pattern in WEIGHTS:
            b = weights(nx, ny, nb, pattern)
            assert b.any() and set(np.unique(b)) <= {0.0, 1.0, 2.0, 3.0}
    nx, ny, nb = LATTICES[0]
    wr = written(nx, ny, nb, 130, weights(nx, ny, nb, "first-tile") != 0).reshape(19, 130)
    assert wr[:16, :128].all() and not wr[16:].any() and not wr[:, 128:].any()
    nx, ny, nb = 33, 5, 5  # the jump lies exactly at I = 128 and J = 16, and one cell further
    b = weights(nx, ny, nb, "jump-on")
    assert b[0, 31] == 1 and b[0, 32] == 3 and b[3, 0] == 1 and b[4, 0] == 2
    b = weights(nx, ny, nb, "jump-across")
    assert b[0, 30] == 1 and b[0, 31] == 3 and b[2, 0] == 1 and b[3, 0] == 2
    b = weights(43, 6, 4, "jump-on")  # H = 3: cell column 42 holds nodes 126 .. 129, cell row 5 nodes 15 .. 18
    assert b[0, 41] == 1 and b[0, 42] == 3 and b[4, 0] == 1 and b[5, 0] == 2


def run_stage(torch, cuda, N, name, forced, f32):
    scalars, stencil_input, pointers, outputs, ref = STAGES[name]
    fn = getattr(N.lib, FAMILY[f32] % name)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bits = np.uint32 if f32 else np.uint64
    for nx, ny, nb in LATTICES:
        stride = stride_of(nx, nb, f32)
        for pattern in WEIGHTS:
            A, w, beta, x, wr = case(nx, ny, nb, pattern, stencil_input, f32)
            want = ref(x, forced)
            bufs = {v: (Buf32(torch, cuda, exact32(x[v], v)) if f32 else Buf(torch, cuda, x[v], 0)) for v in pointers}
            args = [None if (v in ("F", "G") and not forced) else bufs[v].p for v in pointers]
            h_weight = beta.reshape(-1).astype(np.float32 if f32 else np.float64)
            d_weight = torch.from_numpy(h_weight.copy()).to(cuda)
            D = description(N, nx, ny, nb, stride, A, w)
            N.check(fn(C.byref(D), C.c_void_p(d_weight.data_ptr()), *scalars, *args, st), name)
            torch.cuda.synchronize()
            target = {buf: key for key, buf in outputs.items()}
            for v in pointers:
                where = f"{name} lattice=({nx},{ny},{nb}) {pattern} stride={stride} {v}"
                if v in target:
                    got = bufs[v].get()
                    expected = np.where(wr, want[target[v]], x[v])  # an all-zero tile keeps what the vector held
                    expected = exact32(expected, where) if f32 else np.ascontiguousarray(expected)
                    bad = np.flatnonzero(got.view(bits) != expected.view(bits))
                    assert bad.size == 0, f"{where}: {bad.size} entries differ, the first at (I, J) = ({bad[0] % stride}, {bad[0] // stride}): " \
                                          f"{got[bad[0]]} for {expected[bad[0]]}"
                else:
                    assert bufs[v].untouched(), where
            assert np.array_equal(d_weight.cpu().numpy(), h_weight)


@pytest.mark.parametrize("name,forced", [(name, forced) for name in STAGES for forced in (True, False)],
                         ids=lambda v: v if isinstance(v, str) else ("forced" if v else "homogeneous"))
def test_weights_stage_matches_numpy_bit_for_bit(cuda, name, forced):
    import torch

    from cuddhelmholtz_amd import _native as N

    run_stage(torch, cuda, N, name, forced, False)


@pytest.mark.parametrize("name,forced", [(name, forced) for name in STAGES for forced in (True, False)],
                         ids=lambda v: v if isinstance(v, str) else ("forced" if v else "homogeneous"))
def test_f32_weights_stage_matches_numpy_bit_for_bit(cuda, name, forced):
    import torch

    from cuddhelmholtz_amd import _native as N

    run_stage(torch, cuda, N, name, forced, True)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(STAGES))
def test_zero_one_weights_give_the_bits_of_the_cells_kernels(cuda, name, f32):
    """every entry point, forced and homogeneous, the eight flag patterns on the seven lattices: random reals, no tolerance"""
    import torch

    from cuddhelmholtz_amd import _native as N

    dtype, tdtype = (np.float32, torch.float32) if f32 else (np.float64, torch.float64)
    _, _, pointers, outputs, _ = STAGES[name]
    n_scalars = len(STAGES[name][0])
    scalars = (0.0371, 0.8131, -0.5821, 0.0193)[:n_scalars]  # non-dyadic
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    compared = 0
    for nx, ny, nb in LATTICES:
        H = nb - 1
        Lx, Ly, stride = nx * H + 1, ny * H + 1, stride_of(nx, nb, f32)
        rng = np.random.default_rng(100 * nb + nx)
        A, w = rng.standard_normal((nb, nb)), rng.random(nb) + 0.5
        D = description(N, nx, ny, nb, stride, A, w)
        D.cx, D.cy = 1.0 / 0.7, 0.7
        host = {}
        for v in pointers:
            h = rng.standard_normal((Ly, stride)).astype(dtype)
            h[:, Lx:] = 0.0
            host[v] = h.reshape(-1)
        for pattern in PATTERNS:
            present = flags(nx, ny, nb, pattern)
            d_cell = torch.from_numpy(present.reshape(-1).copy()).to(cuda)
            d_weight = torch.from_numpy(present.reshape(-1).astype(dtype)).to(cuda)
            for forced in (True, False):
                got = {}
                for family, table in (("cells", d_cell), ("weights", d_weight)):
                    x = {v: torch.from_numpy(host[v]).to(cuda) for v in pointers}
                    args = [None if (v in ("F", "G") and not forced) else ptr(x[v]) for v in pointers]
                    fn = getattr(N.lib, (CELLS if family == "cells" else FAMILY)[f32] % name)
                    N.check(fn(C.byref(D), ptr(table), *scalars, *args, st), f"{family} {name}")
                    torch.cuda.synchronize()
                    got[family] = x
                for v in pointers:
                    assert torch.equal(got["cells"][v].view(torch.int32 if f32 else torch.int64), got["weights"][v].view(torch.int32 if f32 else torch.int64)), \
                        f"{name} lattice=({nx},{ny},{nb}) {pattern} forced={forced} {v}"
                for v in outputs.values():
                    compared += int((got["weights"][v] != torch.from_numpy(host[v]).to(cuda)).sum())
    assert compared > 1000  # the launches wrote


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_bad_calls_are_refused_and_write_nothing(cuda, f32):
    import torch

    from cuddhelmholtz_amd import _native as N

    nx, ny, nb = 2, 2, 4  # Lx = 7
    stride = 8
    A, w = tables(nb, seed=1)
    x = host_vectors(nx, 6, nb, 28, seed=5)  # room for every description tried, were one of them launched
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pointers = STAGES["rk4_2"][2]
    weight = torch.ones(64, dtype=torch.float32 if f32 else torch.float64, device=cuda)
    make = (lambda v, off: Buf32(torch, cuda, x[v], off)) if f32 else (lambda v, off: Buf(torch, cuda, x[v], off))
    family = FAMILY[f32]

    def attempt(D, swap=None, off=None, absent=(), no_weight=False):
        bufs = {v: make(v, 1 if v == off else 0) for v in pointers}
        args = [None if v in absent else bufs[(swap or {}).get(v, v)].p for v in pointers]
        err = getattr(N.lib, family % "rk4_2")(C.byref(D), None if no_weight else C.c_void_p(weight.data_ptr()), HALF_DT, CS, SN, *args, st)
        torch.cuda.synchronize()
        assert err == 1, (swap, off, absent, no_weight, err)
        assert all(b.untouched() for b in bufs.values())

    good = description(N, nx, ny, nb, stride, A, w)
    attempt(good, swap={"ps_out": "ps"})  # an output that is the stencil input
    attempt(good, off="q")  # pointers off a 16-byte boundary
    attempt(good, off="aq")
    attempt(good, off="F")
    attempt(good, absent=("G",))  # F without G
    attempt(good, absent=("F",))
    attempt(good, absent=("p",))
    attempt(good, no_weight=True)
    attempt(description(N, nx, ny, nb, 7, A, w))  # an odd stride
    attempt(description(N, nx, ny, nb, 4, A, w))  # a stride below Lx = 7
    if f32:
        attempt(description(N, nx, ny, nb, 10, A, w))  # no multiple of 4
    attempt(description(N, nx, ny, 9, 28, A, w))  # n_basis beyond 8
    attempt(description(N, 0, ny, nb, stride, A, w))
    for name, scalars in (("rk2_b", (DT, CS, SN, FILT)), ("rk4_4", (DT, CS, SN, FILT))):  # they write p, q, u, v
        bufs = {v: make(v, 0) for v in STAGES[name][2]}
        args = [bufs["q" if v == "ps" else v].p for v in STAGES[name][2]]
        assert getattr(N.lib, family % name)(C.byref(good), C.c_void_p(weight.data_ptr()), *scalars, *args, st) == 1
        torch.cuda.synchronize()
        assert all(b.untouched() for b in bufs.values())
    for name in STAGES:  # every entry point refuses a null weight
        bufs = {v: make(v, 0) for v in STAGES[name][2]}
        assert getattr(N.lib, family % name)(C.byref(good), None, *STAGES[name][0], *[bufs[v].p for v in STAGES[name][2]], st) == 1
        torch.cuda.synchronize()
        assert all(b.untouched() for b in bufs.values())
