"""kernels/wave_cells.hip and wave_cells_f32.hip (lattice sweeps with missing cells), entry point by entry point through the C ABI,
bit for bit against numpy.

The data is that of test_gpu_wave_lattice_kernels.py: A holds integers in [-4, 4] and is not symmetric, the weights are 1 or 2,
cx = 2, cy = 1/2, vectors hold small integers, invm and every coefficient are powers of two.  Everything the stencil and the stages
form is then exact in float64 (and, asserted here on the CPU, in float32) whatever the order of the operations.  The restatement is
not the kernel's regrouping per node (sL, sR, sB, sA and four flags, the head of wave_cells.hip) but what that regroups: the sum
over the PRESENT cells of the element's own Kronecker sum,
    (K_e p)[b, a] = cx w[b] sum_a' A[a][a'] p[b, a'] + cy w[a] sum_b' A[b][b'] p[b', a]        on the cell's n_basis x n_basis nodes,
which is zero at a node with no present cell around it.  A workgroup whose tile of 128 x 16 nodes has no node in a present cell
writes nothing: there every output must keep the bits it held.

Lattices (nx, ny, n_basis): (43,6,4) 130 x 19 nodes, 2 x 2 tiles, Lx even; (42,5,4) 127 x 16, one tile, Lx odd; (33,5,5) 133 x 21,
where cell edges fall on the tile boundaries I = 128 and J = 16; (70,9,3) and (129,17,2) on the run-time n_basis instantiation with
2 x 2 tiles (n_basis 2 stages the most flags a tile can have); (3,2,8), (2,3,6) small run-time ones.  Flag patterns: every cell; one
cell; a checkerboard (cells that touch at corners only); a random 70 %; only the cells of tile (0, 0) (three wholly void tiles
beside a full one); a hole whose edge lies on the tile boundary where H divides it; a hole that straddles it; holes on the lattice
boundary (a notch at the left edge and the last corner cell).

Void nodes carry invm = 0 and otherwise arbitrary data: their outputs are the stage applied to K p = 0.  Both precisions, the forced
and the homogeneous form; guards and unwritten vectors are compared bitwise; bad calls return 1 and write nothing.  With every cell
present the kernels are compared with the cuddh_hip_wave_lattice_* / cuddh_hip_wave32_* entry points on random reals: the two differ
by the regrouping of the element-boundary diagonal, gate 16 eps times the largest |term| of the node's sum.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_wave_lattice_f32_kernels import Buf32, exact32
from test_gpu_wave_lattice_kernels import CX, CY, STAGES, description, host_vectors, stencil, tables
from test_gpu_wave_stage_kernels import CS, DT, FILT, HALF_DT, SN, Buf

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

TX, TY = 128, 16
LATTICES = [(43, 6, 4), (42, 5, 4), (33, 5, 5), (70, 9, 3), (129, 17, 2), (3, 2, 8), (2, 3, 6)]
PATTERNS = ("all", "one", "checker", "random", "first-tile", "edge", "straddle", "boundary")


def stride_of(nx, nb, f32):
    Lx = nx * (nb - 1) + 1
    return (Lx + 3) // 4 * 4 if f32 else Lx + Lx % 2


@functools.lru_cache(maxsize=None)
def flags(nx, ny, nb, pattern):
    """(ny, nx) uint8, read-only"""
    H = nb - 1
    f = np.ones((ny, nx), dtype=np.uint8)
    aE, bE = TX // H, TY // H  # the cell column / row that begins at the tile boundary (H divides it) or contains it
    if pattern == "one":
        f[:] = 0
        f[ny // 2, nx // 2] = 1
    elif pattern == "checker":
        f[:] = (np.add.outer(np.arange(ny), np.arange(nx)) % 2 == 0)
    elif pattern == "random":
        f[:] = np.random.default_rng(100 * nx + ny).random((ny, nx)) < 0.7
        f[0, 0] = 1
    elif pattern == "first-tile":
        # the cells with a node in tile (0, 0) only, less those with a node in another tile: tiles (1, 0), (0, 1), (1, 1) are void
        f[:] = 0
        f[: max(1, (TY - 1) // H), : max(1, (TX - 1) // H)] = 1
    elif pattern == "edge":
        f[max(bE - 1, 0): bE + 1, aE: aE + 2] = 0
        f[bE: bE + 2, max(aE - 3, 0): aE - 1] = 0
    elif pattern == "straddle":
        f[bE - 1: bE + 1, max(aE - 1, 0): aE + 1] = 0
    elif pattern == "boundary":
        f[1:3, 0:2] = 0
        f[ny - 1, nx - 1] = 0
        f[0, nx // 2] = 0
    if not f.any():
        f[0, 0] = 1
    f.setflags(write=False)
    return f


def stencil_cells(nx, ny, nb, stride, A, w, present, p):
    """K p on the padded lattice vector p: the sum of the present cells' element matrices; zero at void nodes and in the padding"""
    H = nb - 1
    Ly = ny * H + 1
    P, K = p.reshape(Ly, stride), np.zeros((Ly, stride))
    for b, a in zip(*np.nonzero(present)):
        sl = (slice(b * H, b * H + nb), slice(a * H, a * H + nb))
        loc = P[sl]
        K[sl] += CX * w[:, None] * (loc @ A.T) + CY * w[None, :] * (A @ loc)
    return K.reshape(-1)


def largest_term(nx, ny, nb, stride, A, w, p):
    """per node, the largest |term| of the sum that K p is, every cell present"""
    H = nb - 1
    Ly = ny * H + 1
    P, big = np.abs(p.reshape(Ly, stride)), np.zeros((Ly, stride))
    absA = np.abs(A)
    for b in range(ny):
        for a in range(nx):
            sl = (slice(b * H, b * H + nb), slice(a * H, a * H + nb))
            loc = P[sl]
            tx = CX * w[:, None, None] * absA[None, :, :] * loc[:, None, :]  # [b, a, a']
            ty = CY * w[None, :, None] * (absA[:, None, :] * loc.T[None, :, :])  # [b, a, b']
            big[sl] = np.maximum(big[sl], np.maximum(tx.max(axis=2), ty.max(axis=2)))
    return big.reshape(-1)


def written(nx, ny, nb, stride, present):
    """(Ly * stride) bools: the slots of the tiles that have a node in a present cell"""
    H = nb - 1
    Lx, Ly = nx * H + 1, ny * H + 1
    out = np.zeros((Ly, stride), dtype=bool)
    for ty0 in range(0, Ly, TY):
        for tx0 in range(0, stride, TX):
            a_lo, a_hi = max(0, -(-tx0 // H) - 1), min(nx - 1, min(tx0 + TX - 1, Lx - 1) // H)
            b_lo, b_hi = max(0, -(-ty0 // H) - 1), min(ny - 1, min(ty0 + TY - 1, Ly - 1) // H)
            out[ty0: ty0 + TY, tx0: tx0 + TX] = present[b_lo: b_hi + 1, a_lo: a_hi + 1].any()
    return out.reshape(-1)


def void_nodes(nx, ny, nb, stride, present):
    """(Ly * stride) bools: lattice nodes (not padding) with no present cell around them"""
    H = nb - 1
    Lx, Ly = nx * H + 1, ny * H + 1
    covered = np.zeros((Ly, stride), dtype=bool)
    for b, a in zip(*np.nonzero(present)):
        covered[b * H: b * H + nb, a * H: a * H + nb] = True
    covered[:, Lx:] = True
    return ~covered.reshape(-1)


@functools.lru_cache(maxsize=None)
def case(nx, ny, nb, pattern, stencil_input, f32):
    """(A, w, flags, vectors with the stencil of `stencil_input` as "w", written slots), computed once and never changed"""
    stride = stride_of(nx, nb, f32)
    A, w = tables(nb, seed=nb)
    present = flags(nx, ny, nb, pattern)
    x = host_vectors(nx, ny, nb, stride, seed=1000 * nx + 10 * ny + nb)
    x["invm"] = np.where(void_nodes(nx, ny, nb, stride, present), 0.0, x["invm"])
    x["w"] = stencil_cells(nx, ny, nb, stride, A, w, present, x[stencil_input])
    assert not x["w"][void_nodes(nx, ny, nb, stride, present)].any()
    if f32:
        exact32(x["w"], "the stencil")
    for v in x.values():
        v.setflags(write=False)
    return A, w, present, x, written(nx, ny, nb, stride, present)


def test_the_restatement_is_the_lattice_stencil_when_every_cell_is_present():
    """(no device) the element sum against test_gpu_wave_lattice_kernels.stencil, and the patterns are what the docstring says"""
    for nx, ny, nb in LATTICES:
        stride = stride_of(nx, nb, False)
        A, w = tables(nb, seed=nb)
        p = host_vectors(nx, ny, nb, stride, seed=3)["p"]
        assert np.array_equal(stencil_cells(nx, ny, nb, stride, A, w, flags(nx, ny, nb, "all"), p), stencil(nx, ny, nb, stride, A, w, p))
    nx, ny, nb = LATTICES[0]
    wr = written(nx, ny, nb, 130, flags(nx, ny, nb, "first-tile")).reshape(19, 130)
    assert wr[:16, :128].all() and not wr[16:].any() and not wr[:, 128:].any()
    assert written(nx, ny, nb, 130, flags(nx, ny, nb, "one")).reshape(19, 130)[:16, :128].all()
    for pattern in PATTERNS[1:]:
        assert 0 < flags(nx, ny, nb, pattern).sum() < nx * ny
    nx, ny, nb = 33, 5, 5  # a hole that begins exactly at I = 128, and one that ends exactly at J = 16
    f = flags(nx, ny, nb, "edge")
    assert f[3, 31] == 1 and f[3, 32] == 0 and f[4, 30] == 0 and f[3, 30] == 1


def run_stage(torch, cuda, N, name, forced, f32):
    scalars, stencil_input, pointers, outputs, ref = STAGES[name]
    fn = getattr(N.lib, f"cuddh_hip_wave_cells32_{name}" if f32 else f"cuddh_hip_wave_cells_{name}_f64")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bits = np.uint32 if f32 else np.uint64
    for nx, ny, nb in LATTICES:
        stride = stride_of(nx, nb, f32)
        for pattern in PATTERNS:
            A, w, present, x, wr = case(nx, ny, nb, pattern, stencil_input, f32)
            want = ref(x, forced)
            bufs = {v: (Buf32(torch, cuda, exact32(x[v], v)) if f32 else Buf(torch, cuda, x[v], 0)) for v in pointers}
            args = [None if (v in ("F", "G") and not forced) else bufs[v].p for v in pointers]
            d_cell = torch.from_numpy(present.reshape(-1).copy()).to(cuda)
            D = description(N, nx, ny, nb, stride, A, w)
            N.check(fn(C.byref(D), C.c_void_p(d_cell.data_ptr()), *scalars, *args, st), name)
            torch.cuda.synchronize()
            target = {buf: key for key, buf in outputs.items()}
            for v in pointers:
                where = f"{name} lattice=({nx},{ny},{nb}) {pattern} stride={stride} {v}"
                if v in target:
                    got = bufs[v].get()
                    expected = np.where(wr, want[target[v]], x[v])  # a void tile keeps what the vector held
                    expected = exact32(expected, where) if f32 else np.ascontiguousarray(expected)
                    bad = np.flatnonzero(got.view(bits) != expected.view(bits))
                    assert bad.size == 0, f"{where}: {bad.size} entries differ, the first at (I, J) = ({bad[0] % stride}, {bad[0] // stride}): " \
                                          f"{got[bad[0]]} for {expected[bad[0]]}"
                else:
                    assert bufs[v].untouched(), where
            assert np.array_equal(d_cell.cpu().numpy(), present.reshape(-1))


@pytest.mark.parametrize("name,forced", [(name, forced) for name in STAGES for forced in (True, False)],
                         ids=lambda v: v if isinstance(v, str) else ("forced" if v else "homogeneous"))
def test_cells_stage_matches_numpy_bit_for_bit(cuda, name, forced):
    import torch

    from cuddhelmholtz_amd import _native as N

    run_stage(torch, cuda, N, name, forced, False)


@pytest.mark.parametrize("name,forced", [(name, forced) for name in STAGES for forced in (True, False)],
                         ids=lambda v: v if isinstance(v, str) else ("forced" if v else "homogeneous"))
def test_f32_cells_stage_matches_numpy_bit_for_bit(cuda, name, forced):
    import torch

    from cuddhelmholtz_amd import _native as N

    run_stage(torch, cuda, N, name, forced, True)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_all_present_agrees_with_the_lattice_kernels_on_random_reals(cuda, f32):
    """rk4_1 with q = 0, Hi = 0, invm = 1 and no load writes aq = K p itself"""
    import torch

    from cuddhelmholtz_amd import _native as N

    dtype, tdtype = (np.float32, torch.float32) if f32 else (np.float64, torch.float64)
    eps = float(np.finfo(dtype).eps)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    worst = 0.0
    for nx, ny, nb in ((43, 6, 4), (42, 5, 4), (33, 5, 5)):
        H = nb - 1
        Lx, Ly, stride = nx * H + 1, ny * H + 1, stride_of(nx, nb, f32)
        rng = np.random.default_rng(nb + nx)
        A, w = rng.standard_normal((nb, nb)), rng.random(nb) + 0.5
        # the tables as the kernels see them: float32 tables are rounded from the doubles
        p = rng.standard_normal((Ly, stride)).astype(dtype)
        p[:, Lx:] = 0.0
        p = p.reshape(-1)
        D = description(N, nx, ny, nb, stride, A, w)
        x = {"p": torch.from_numpy(p).to(cuda), "q": torch.zeros(Ly * stride, dtype=tdtype, device=cuda)}
        x["Hi"] = torch.zeros_like(x["q"])
        x["invm"] = torch.ones_like(x["q"])
        cell = torch.ones(nx * ny, dtype=torch.uint8, device=cuda)
        got = {}
        for family in ("cells", "lattice"):
            out = {v: torch.zeros_like(x["q"]) for v in ("ps", "qs", "aq", "ap")}
            ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
            tail = (0.37, 0.8, -0.6, ptr(x["p"]), ptr(x["q"]), ptr(x["invm"]), ptr(x["Hi"]), None, None, ptr(out["ps"]), ptr(out["qs"]), ptr(out["aq"]),
                    ptr(out["ap"]), st)
            if family == "cells":
                fn = N.lib.cuddh_hip_wave_cells32_rk4_1 if f32 else N.lib.cuddh_hip_wave_cells_rk4_1_f64
                N.check(fn(C.byref(D), ptr(cell), *tail), "cells rk4_1")
            else:
                fn = N.lib.cuddh_hip_wave32_rk4_1 if f32 else N.lib.cuddh_hip_wave_lattice_rk4_1_f64
                N.check(fn(C.byref(D), *tail), "lattice rk4_1")
            torch.cuda.synchronize()
            got[family] = out["aq"].cpu().numpy().astype(np.float64)
        big = largest_term(nx, ny, nb, stride, A, w, p.astype(np.float64))
        ratio = np.abs(got["cells"] - got["lattice"]) / np.where(big > 0, eps * big, 1.0)
        assert np.all(got["cells"][big == 0] == 0) and np.all(got["lattice"][big == 0] == 0)
        worst = max(worst, float(ratio.max()))
        assert float(np.abs(got["lattice"]).max()) > 1.0
    print(f"wave_cells against wave_lattice, every cell present, {'f32' if f32 else 'f64'}: largest difference {worst:.2f} eps x largest |term| "
          f"(gate 16)")
    assert worst < 16.0


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
    cell = torch.ones(64, dtype=torch.uint8, device=cuda)
    make = (lambda v, off: Buf32(torch, cuda, x[v], off)) if f32 else (lambda v, off: Buf(torch, cuda, x[v], off))
    family = "cuddh_hip_wave_cells32_%s" if f32 else "cuddh_hip_wave_cells_%s_f64"

    def attempt(D, swap=None, off=None, absent=(), no_cell=False):
        bufs = {v: make(v, 1 if v == off else 0) for v in pointers}
        args = [None if v in absent else bufs[(swap or {}).get(v, v)].p for v in pointers]
        err = getattr(N.lib, family % "rk4_2")(C.byref(D), None if no_cell else C.c_void_p(cell.data_ptr()), HALF_DT, CS, SN, *args, st)
        torch.cuda.synchronize()
        assert err == 1, (swap, off, absent, no_cell, err)
        assert all(b.untouched() for b in bufs.values())

    good = description(N, nx, ny, nb, stride, A, w)
    attempt(good, swap={"ps_out": "ps"})  # an output that is the stencil input
    attempt(good, off="q")  # pointers off a 16-byte boundary
    attempt(good, off="aq")
    attempt(good, off="F")
    attempt(good, absent=("G",))  # F without G
    attempt(good, absent=("F",))
    attempt(good, absent=("p",))
    attempt(good, no_cell=True)
    attempt(description(N, nx, ny, nb, 7, A, w))  # an odd stride
    attempt(description(N, nx, ny, nb, 4, A, w))  # a stride below Lx = 7
    if f32:
        attempt(description(N, nx, ny, nb, 10, A, w))  # no multiple of 4
    attempt(description(N, nx, ny, 9, 28, A, w))  # n_basis beyond 8
    attempt(description(N, 0, ny, nb, stride, A, w))
    for name, scalars in (("rk2_b", (DT, CS, SN, FILT)), ("rk4_4", (DT, CS, SN, FILT))):  # they write p, q, u, v
        bufs = {v: make(v, 0) for v in STAGES[name][2]}
        args = [bufs["q" if v == "ps" else v].p for v in STAGES[name][2]]
        assert getattr(N.lib, family % name)(C.byref(good), C.c_void_p(cell.data_ptr()), *scalars, *args, st) == 1
        torch.cuda.synchronize()
        assert all(b.untouched() for b in bufs.values())
