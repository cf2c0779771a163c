"""krylov_update_{f64,f32} of kernels/blas1.hip through the C ABI, bit for bit against a numpy restatement on exact integers.

    d[i] = sum_j coef[j] V[j ldv + i] + sum_p coef[nv + p] Z[p ldz + i];   dx[i] = d[i];   x[i] += d[i];
    pout[b] = workgroup b's partial sum of d^2  (row 0 of a cgs partial buffer: cgs_reduce with k1 = 0 finishes it)

Sizes (N = elements of a 16-byte vector, a tile = 1024 vectors): 0, 1, 3; tile - 1, tile, tile + 1; three tiles, five vectors and
a scalar tail; beyond that one size with a workgroup's second tile and one at the non-temporal threshold (64 MiB per vector).
Columns: nv in {1, 2, KC - 1, KC, KC + 1, 20, 512 - nz} (KC = 4 columns per register chunk), nz in {0, 1, 3}.  Placements:
everything aligned with padded leading dimensions; x, dx, V or Z off by one element; ldv = ldz = n; ldv or ldz with remainder 1
modulo N -- all but the first must take the element-wise path for every operand and still match.

Inputs: every element has at most two nonzero column entries (+-1, in two different columns), coefficients +-(1 + j mod 7), x in
{-3..3}: |d| <= 14 and every sum stays below the exactness limit of the type (asserted), so every summation order gives the same
bits.  Buffers carry NaN guards on both sides (checked on every read-back), the gaps between columns hold a value that would
change every sum, outputs start as a sentinel.
"""
import ctypes as C

import numpy as np
import pytest

import blas1_reference as br
import cgs2_reference as cr
from test_gpu_cgs2_kernels import GAP, ROW, SENT, Buf, Ctx, leading_dimension, same_bits

pytestmark = pytest.mark.gpu

#             x  dx V  Z  ldv       ldz
PLACEMENTS = [(0, 0, 0, 0, "padded", "padded"), (1, 0, 0, 0, "padded", "padded"), (0, 1, 0, 0, "padded", "padded"), (0, 0, 1, 0, "padded", "padded"),
              (0, 0, 0, 1, "padded", "padded"), (0, 0, 0, 0, "tight", "tight"), (0, 0, 0, 0, "odd", "padded"), (0, 0, 0, 0, "padded", "odd")]
NVS = (1, 2, cr.KC - 1, cr.KC, cr.KC + 1, 20)
NZS = (0, 1, 3)


@pytest.fixture(scope="module")
def ctx(cuda):
    return Ctx(cuda)


def sizes(dtype):
    s = br.sizes(dtype)
    return {"small": [0, 1, 3], "tile": s["tile"], "ragged": s["ragged"]}


def exact_update(n, dtype, nv, nz, rng):
    """(coef, columns as int8 (nv + nz, n), x, d, sum d^2) in integers; see the module docstring"""
    nc = nv + nz
    coef = np.array([(1 + j % 7) * (-1 if (j // 7 + j) % 2 else 1) for j in range(nc)], dtype=np.int64)
    cols = np.zeros((nc, n), dtype=np.int8)
    x = rng.integers(-3, 4, n).astype(np.int64)
    d = np.zeros(n, dtype=np.int64)
    if n:
        q = min(1.0, br.EXACT_LIMIT[dtype] / 4 / (196.0 * n))
        active = rng.random(n) < q
        for idx in br.marked(n, dtype).values():
            active[np.asarray(idx, dtype=np.int64)] = True
        i = np.flatnonzero(active)
        j1 = rng.integers(0, nc, len(i))
        cols[j1, i] = rng.choice(np.array([-1, 1], dtype=np.int8), len(i))
        if nc > 1:
            j2 = (j1 + 1 + rng.integers(0, nc - 1, len(i))) % nc
            cols[j2, i] = rng.choice(np.array([-1, 1], dtype=np.int8), len(i))
        for j in range(nc):
            d += coef[j] * cols[j].astype(np.int64)
    dd = int(np.dot(d, d))
    assert dd <= br.EXACT_LIMIT[dtype] // 4 and (n == 0 or np.max(np.abs(d)) <= 14)
    return coef, cols, x, d, dd


def column_array(cols, n, ld, dtype):
    """the columns ld apart (the last one n long), GAP between them; one GAP element when there is no column"""
    k = len(cols)
    if k == 0:
        return np.full(1, GAP, dtype=br.NP[dtype])
    flat = np.full(ld * (k - 1) + n, GAP, dtype=br.NP[dtype])
    for j in range(k):
        flat[j * ld:j * ld + n] = cols[j]
    return flat


def update(ctx, dtype, n, x, dx, V, ldv, nv, Z, ldz, nz, coef, pout, raw=False):
    f = ctx.raw if raw else ctx.call
    return f(f"krylov_update_{dtype}", n, x, dx, V, ldv, nv, Z, ldz, nz, coef, pout)


def check_update_exact(ctx, dtype, n, nv, nz, placement, seed):
    T = br.NP[dtype]
    ox, od, ov, oz, mv, mz = placement
    ldv, ldz = leading_dimension(n, dtype, mv), leading_dimension(n, dtype, mz)
    where = f"{dtype} n={n} nv={nv} nz={nz} placement={placement} ldv={ldv} ldz={ldz}"
    coef, cols, x0, d, dd = exact_update(n, dtype, nv, nz, np.random.default_rng(seed))
    fv, fz = column_array(cols[:nv], n, ldv, dtype), column_array(cols[nv:], n, ldz, dtype)
    bx, bd = Buf(ctx, dtype, n, ox, x0), Buf(ctx, dtype, n, od, np.full(n, SENT))
    bv, bz = Buf(ctx, dtype, len(fv), ov, fv), Buf(ctx, dtype, len(fz), oz, fz)
    bc = Buf(ctx, dtype, nv + nz, data=coef)
    bp, bs = Buf(ctx, dtype, ROW, data=np.full(ROW, SENT)), Buf(ctx, dtype, 2, data=np.full(2, SENT))
    assert update(ctx, dtype, n, bx.p, bd.p, bv.p, ldv, nv, bz.p if nz else None, ldz, nz, bc.p, bp.p) == 0
    gx, gd, gp = bx.get(), bd.get(), bp.get()  # (get: the canaries on both sides of x, dx and the partials are intact)
    assert same_bits(gd, d, dtype), f"{where}: dx differs at {np.flatnonzero(gd != d)[:8]}"
    assert same_bits(gx, x0 + d, dtype), f"{where}: x differs at {np.flatnonzero(gx != x0 + d)[:8]}"
    if n == 0:
        assert np.all(gp == T(SENT)), f"{where}: n = 0 wrote partial sums"
        return
    g = br.mgs_grid(n)
    assert ctx.lib.cuddh_hip_cgs_partials(n) == g
    part = gp[:g]
    assert np.all(part == np.rint(part)) and float(np.sum(part.astype(np.float64))) == float(dd), f"{where}: partials sum to {np.sum(part.astype(np.float64))}, not {dd}"
    assert np.all(gp[g:] == T(SENT)), f"{where}: slots behind the {g} workgroups' were written"
    ctx.call(f"cgs_reduce_{dtype}", n, 0, bp.p, bs.p)
    assert same_bits(bs.get(), [T(dd), T(SENT)], dtype), f"{where}: cgs_reduce gives {bs.get()}, not {dd}"
    assert same_bits(bv.get(), fv, dtype) and same_bits(bz.get(), fz, dtype) and same_bits(bc.get(), coef, dtype), f"{where}: an input changed"


@pytest.mark.parametrize("group", ["small", "tile", "ragged"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_update_exact(ctx, dtype, group):
    """dx, x and the partial sums of |dx|^2 bit for bit, cgs_reduce(k1 = 0) on them, nothing written outside: every size of the
    group with every nv below the cap, nz and placement of the module docstring"""
    for n in sizes(dtype)[group]:
        for nv in NVS:
            for nz in NZS:
                for placement in PLACEMENTS:
                    check_update_exact(ctx, dtype, n, nv, nz, placement, seed=n + 31 * nv + nz)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_update_exact_with_512_columns(ctx, dtype):
    """nv = 512 - nz: the whole coefficient table, on the vector path, with x off by one element and with an odd ldv"""
    for n in (3, sizes(dtype)["tile"][2], sizes(dtype)["ragged"][0]):
        for nz in NZS:
            for placement in (PLACEMENTS[0], PLACEMENTS[1], PLACEMENTS[6]):
                check_update_exact(ctx, dtype, n, cr.KMAX - nz, nz, placement, seed=n + nz)


@pytest.mark.parametrize("group", ["further", "nt"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_update_exact_large(ctx, dtype, group):
    """further: more than 1024 tiles, a workgroup's second tile; nt: N - 1 elements past the 64 MiB from which the kernel streams
    with the non-temporal hint (the last size below it is covered by every other test).  nv = 3, nz = 1, aligned and with odd ldv."""
    n = br.sizes(dtype)["further"][0] if group == "further" else br.sizes(dtype)["nt"][1] + br.PACK[dtype] - 1
    if group == "further":
        assert br.marked(n, dtype)["beyond"]
    else:
        assert n * np.dtype(br.NP[dtype]).itemsize >= br.NT_BYTES
    for placement in (PLACEMENTS[0], PLACEMENTS[6]) if group == "further" else (PLACEMENTS[0],):
        check_update_exact(ctx, dtype, n, 3, 1, placement, seed=9)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_invalid_arguments_launch_nothing(ctx, dtype):
    """nv < 1, nz < 0, nv + nz > 512, ldv < n with nv > 1, ldz < n with nz > 1, n < 0: an error status and nothing written;
    ldv < n with one column and nv + nz = 512 are accepted"""
    T = br.NP[dtype]
    n = 64
    x0 = np.arange(n, dtype=T)
    bx, bd = Buf(ctx, dtype, n, 0, x0), Buf(ctx, dtype, n, 0, np.full(n, SENT))
    bv, bz = Buf(ctx, dtype, cr.KMAX * n, 0, np.ones(cr.KMAX * n, dtype=T)), Buf(ctx, dtype, 3 * n, 0, np.ones(3 * n, dtype=T))
    bc, bp = Buf(ctx, dtype, cr.KMAX + 1, data=np.ones(cr.KMAX + 1)), Buf(ctx, dtype, ROW, data=np.full(ROW, SENT))
    bad = [dict(nv=0), dict(nv=-1), dict(nz=-1), dict(nv=cr.KMAX, nz=1), dict(nv=cr.KMAX + 1, nz=0), dict(nv=2, ldv=n - 1), dict(nz=2, ldz=n - 1),
           dict(nv=2, ldv=-n), dict(n=-1)]
    for kw in bad:
        a = dict(n=n, nv=2, nz=1, ldv=n, ldz=n)
        a.update(kw)
        rc = update(ctx, dtype, a["n"], bx.p, bd.p, bv.p, a["ldv"], a["nv"], bz.p, a["ldz"], a["nz"], bc.p, bp.p, raw=True)
        assert rc != 0, kw
    assert update(ctx, dtype, 0, bx.p, bd.p, bv.p, n, 2, bz.p, n, 1, bc.p, bp.p, raw=True) == 0
    ctx.torch.cuda.synchronize()
    assert same_bits(bx.get(), x0, dtype) and np.all(bd.get() == T(SENT)) and np.all(bp.get() == T(SENT))
    # accepted: a single column needs no leading dimension; 512 columns in all
    assert update(ctx, dtype, n, bx.p, bd.p, bv.p, 0, 1, bz.p, 0, 1, bc.p, bp.p) == 0
    assert np.all(bd.get() == T(2)) and same_bits(bx.get(), x0 + 2, dtype)
    assert update(ctx, dtype, n, bx.p, bd.p, bv.p, n, cr.KMAX - 3, bz.p, n, 3, bc.p, bp.p) == 0
    assert np.all(bd.get() == T(cr.KMAX)) and same_bits(bx.get(), x0 + 2 + cr.KMAX, dtype)
