"""cmgs_stage_{f64,f32} and ckrylov_update_{f64,f32} of kernels/blas1.hip (complex arithmetic on split [Re; Im] vectors) through the
C ABI, bit for bit against numpy on exact integers.

    stage:   c = sum(pin row 0) + i sum(pin row 1) -> hout[0], hout[1];   w <- w - c v_prev;
             pout row 0 / 1 <- partial sums of Re / Im <v_next, w>   (v_next NULL, the finish stage: row 0 <- those of |w|^2, row 1 <- 0,
             and mgs_finish on the 2 h scalars turns row 0 into the norm and normalises)
    update:  x <- x + sum_j (coef[2 j] + i coef[2 j + 1]) v_j

Sizes h (complex entries; N = elements of a 16-byte vector; a tile = 512 vectors of each half): 1, 2, 3, 63, 64, 65, 255, 257; one h
either side of a tile (512 N), of two tiles, and of 1024 (where the grid takes a second workgroup); three tiles and five vectors,
and one more (the element-wise path: h is no multiple of N); more than 1024 tiles (a workgroup's second tile); for the update one h
either side of the non-temporal threshold (2 h scalars = 64 MiB).  Placements: aligned, and w / x, v_prev, v_next / V off by one
element from a 16-byte boundary; for the update also tight and odd leading dimensions.  k1 in {1, 2, 20} for the update.

Inputs are small integers: w in {-2..2}, v_prev and v_next in {-1, 0, 1}, c in {-3..3}^2, so |w - c v_prev| <= 14 per part; where the
sums over h would pass the exactness limit of the type (2^24, 2^53) w and v_prev are nonzero only at a random subset and at the
marked places (first element, the tile boundary, the last full vector, the last element, tile 1024).  Every product and sum is
then exact in the type and the order of summation cannot matter.  Buffers carry NaN guards on both sides (checked on every
read-back), outputs start as a sentinel, partial slots beyond the workgroups' hold a value that would change every sum.
"""
import ctypes as C

import numpy as np
import pytest

import blas1_reference as br
import cgmres_reference as cg
from test_gpu_cgs2_kernels import GAP, SENT, Buf, Ctx, same_bits

pytestmark = pytest.mark.gpu

ROW = cg.CPLX_ROW
STAGE_OFFSETS = br.MGS_OFFSETS  # (w, vprev, vnext)
#                     x  V  ldv
UPDATE_PLACEMENTS = [(0, 0, "padded"), (1, 0, "padded"), (0, 1, "padded"), (1, 1, "padded"), (0, 0, "tight"), (0, 0, "odd")]
K1S = (1, 2, 20)


@pytest.fixture(scope="module")
def ctx(cuda):
    return Ctx(cuda)


def split(re, im, dtype):
    return np.concatenate([re, im]).astype(br.NP[dtype])


def exact_stage(h, dtype, rng):
    """(w_r, w_i, p_r, p_i, n_r, n_i) as int64; see the module docstring"""
    q = min(1.0, br.EXACT_LIMIT[dtype] / 4 / (2 * 14 * 14 * h))
    active = rng.random(h) < q
    active[cg.marked(h, dtype)] = True
    w = rng.integers(-2, 3, (2, h)) * active
    p = rng.integers(-1, 2, (2, h)) * active
    for i in cg.marked(h, dtype):  # nonzero there, real and imaginary part different
        w[:, i], p[:, i] = (2, -1), (1, -1)
    nx = rng.integers(-1, 2, (2, h))
    return w[0], w[1], p[0], p[1], nx[0], nx[1]


def stage_ref(w, p, nx, c):
    """integers: the new (w_r, w_i) and the two sums the stage leaves behind"""
    wr, wi = w
    if p is not None:
        wr, wi = wr - (c[0] * p[0] - c[1] * p[1]), wi - (c[0] * p[1] + c[1] * p[0])
    if nx is None:
        return (wr, wi), int(np.dot(wr, wr) + np.dot(wi, wi)), 0
    return (wr, wi), int(np.dot(nx[0], wr) + np.dot(nx[1], wi)), int(np.dot(nx[0], wi) - np.dot(nx[1], wr))


def partial_rows(g, c, rng):
    """2 x 1024 partials: row r sums to c[r] over its first g slots, the slots behind hold SENT"""
    part = np.full(2 * ROW, SENT)
    for r in range(2):
        v = rng.integers(-2, 3, g)
        v[0] += c[r] - int(v.sum())
        part[r * ROW:r * ROW + g] = v
    return part


def check_stage_exact(ctx, dtype, h, offs, seed):
    T = br.NP[dtype]
    ow, op, on = offs
    where = f"{dtype} h={h} offsets={offs}"
    rng = np.random.default_rng(seed)
    wr, wi, pr, pi, nr, ni = exact_stage(h, dtype, rng)
    g = cg.cplx_grid(h)
    assert ctx.lib.cuddh_hip_cgs_partials(2 * h) == g and ctx.lib.cuddh_hip_cmgs_ws_bytes() == 4 * ROW * 8
    w0 = split(wr, wi, dtype)
    bw, bp, bn = Buf(ctx, dtype, 2 * h, ow, w0), Buf(ctx, dtype, 2 * h, op, split(pr, pi, dtype)), Buf(ctx, dtype, 2 * h, on, split(nr, ni, dtype))
    ws = Buf(ctx, dtype, 4 * ROW)
    hc = Buf(ctx, dtype, 4)
    c = (int(rng.integers(1, 4)) * (-1) ** seed, int(rng.integers(-3, 4)))

    for prev, nxt in ((False, True), (True, True), (True, False), (False, False)):
        what = f"stage prev={prev} next={nxt} {where}"
        pin = partial_rows(g, c, rng)
        ws.set(np.concatenate([pin, np.full(2 * ROW, SENT)]))
        hc.set(np.full(4, SENT))
        bw.set(w0)
        (er, ei), sr, si = stage_ref((wr, wi), (pr, pi) if prev else None, (nr, ni) if nxt else None, c)
        assert max(np.max(np.abs(er)), np.max(np.abs(ei))) <= 14
        assert ctx.call(f"cmgs_stage_{dtype}", h, bw.p, bp.p if prev else None, bn.p if nxt else None, ws.at(0), ws.at(2 * ROW), hc.at(1)) == 0
        got_w, got_ws, got_h = bw.get(), ws.get(), hc.get()
        assert same_bits(got_w, split(er, ei, dtype), dtype), f"{what}: w differs at {np.flatnonzero(got_w != split(er, ei, dtype))[:8]}"
        assert same_bits(got_h, [SENT, c[0], c[1], SENT] if prev else np.full(4, SENT), dtype), f"{what}: hout {got_h}"
        assert same_bits(got_ws[:2 * ROW], pin, dtype), f"{what}: the input partials changed"
        for r, want in ((0, sr), (1, si)):
            row = got_ws[(2 + r) * ROW:(3 + r) * ROW]
            assert np.all(row[:g] == np.rint(row[:g])) and float(np.sum(row[:g].astype(np.float64))) == float(want), \
                f"{what}: row {r} sums to {np.sum(row[:g].astype(np.float64))}, not {want}"
            assert np.all(row[g:] == T(SENT)), f"{what}: slots behind the {g} workgroups' were written in row {r}"
        if not nxt:
            assert not np.any(got_ws[3 * ROW:3 * ROW + g]), f"{what}: the imaginary row of |w|^2 is not zero"
        if prev and not nxt and sr > 0:
            # the finish: mgs_finish on the 2 h scalars reads row 0 -- the norm is the correctly rounded root of the integer
            assert ctx.call(f"mgs_finish_{dtype}", 2 * h, bw.p, ws.at(2 * ROW), hc.at(3)) == 0
            nrm = hc.get()[3]
            assert same_bits([nrm], [np.sqrt(T(sr))], dtype), f"finish {where}: norm {nrm!r}, |w|^2 = {sr}"
            W = br.wide(dtype)
            want = split(er, ei, dtype).astype(W) / W(nrm)
            assert np.all(np.abs(bw.get().astype(W) - want) <= br.quotient_bound(want, dtype)), f"finish {where}: w / norm"
    assert same_bits(bp.get(), split(pr, pi, dtype), dtype) and same_bits(bn.get(), split(nr, ni, dtype), dtype), f"{where}: an input changed"


@pytest.mark.parametrize("group", ["small", "tile", "ragged"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_stage_and_finish_exact(ctx, dtype, group):
    """the four variants of cmgs_stage (first stage, projection stage, finish stage, norm only) and mgs_finish behind the finish
    stage: hout is the coefficient, every element of the new w is w - c v_prev, the partial rows sum to Re and Im <v_next, w> (or
    |w|^2 and 0), nothing else is written -- every size of the group under every placement"""
    for h in cg.sizes(dtype)[group]:
        for offs in STAGE_OFFSETS:
            check_stage_exact(ctx, dtype, h, offs, seed=h + sum(offs))


@pytest.mark.parametrize("offs", [(0, 0, 0), (0, 1, 0)])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_stage_and_finish_exact_further_tiles(ctx, dtype, offs):
    """more than 1024 tiles: a workgroup's second tile, with marked nonzeros in tile 1024"""
    (h,) = cg.sizes(dtype)["further"]
    assert br.PACK[dtype] * cg.CTILE * br.MAX_PARTIALS + 3 in cg.marked(h, dtype)
    check_stage_exact(ctx, dtype, h, offs, seed=5)


# ================================================================== the update
def leading_dimension(h, dtype, mode):
    N = br.PACK[dtype]
    padded = -(-2 * h // N) * N
    return {"padded": padded, "tight": 2 * h, "odd": padded + 1}[mode]


def check_update_exact(ctx, dtype, h, k1, placement, seed):
    ox, ov, mode = placement
    ldv = leading_dimension(h, dtype, mode)
    where = f"{dtype} h={h} k1={k1} placement={placement} ldv={ldv}"
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, (2, h), dtype=np.int8)
    V = rng.integers(-1, 2, (k1, 2, h), dtype=np.int8)
    for i in cg.marked(h, dtype):
        V[:, :, i] = (1, -1)
    y = np.array([[(1 + j % 3) * (-1 if j % 2 else 1), (j + seed) % 3 - 1] for j in range(k1)], dtype=np.int64)
    y[0, 1] = 2  # (an imaginary part that is never zero)
    er, ei = x[0].astype(np.int32), x[1].astype(np.int32)
    for j in range(k1):
        vr, vi, yr, yi = V[j, 0].astype(np.int32), V[j, 1].astype(np.int32), int(y[j, 0]), int(y[j, 1])
        er += yr * vr - yi * vi
        ei += yr * vi + yi * vr
    assert max(np.max(np.abs(er)), np.max(np.abs(ei))) < 2 ** 10
    flat = np.full(ldv * (k1 - 1) + 2 * h, GAP, dtype=br.NP[dtype])
    for j in range(k1):
        flat[j * ldv:j * ldv + 2 * h] = split(V[j, 0], V[j, 1], dtype)
    bx, bv, bc = Buf(ctx, dtype, 2 * h, ox, split(x[0], x[1], dtype)), Buf(ctx, dtype, len(flat), ov, flat), Buf(ctx, dtype, 2 * k1, data=y.reshape(-1))
    assert ctx.call(f"ckrylov_update_{dtype}", h, bx.p, bv.p, ldv, k1, bc.p) == 0
    got = bx.get()  # (get: the guards on both sides are intact)
    assert same_bits(got, split(er, ei, dtype), dtype), f"{where}: x differs at {np.flatnonzero(got != split(er, ei, dtype))[:8]}"
    assert same_bits(bv.get(), flat, dtype) and same_bits(bc.get(), y.reshape(-1), dtype), f"{where}: an input changed"


@pytest.mark.parametrize("group", ["small", "tile", "ragged"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_update_exact(ctx, dtype, group):
    """x + sum_j y_j v_j bit for bit and nothing written outside x: every size of the group with k1 in {1, 2, 20} under every placement"""
    for h in cg.sizes(dtype)[group]:
        for k1 in K1S:
            for placement in UPDATE_PLACEMENTS:
                check_update_exact(ctx, dtype, h, k1, placement, seed=h + 31 * k1)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_update_exact_with_512_columns(ctx, dtype):
    """k1 = 512: the whole coefficient table, on the vector path, with x off by one element and with an odd ldv"""
    for h in (3, cg.sizes(dtype)["tile"][1]):
        for placement in (UPDATE_PLACEMENTS[0], UPDATE_PLACEMENTS[1], UPDATE_PLACEMENTS[5]):
            check_update_exact(ctx, dtype, h, cg.KMAX, placement, seed=h)


@pytest.mark.parametrize("group", ["further", "nt"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_update_exact_large(ctx, dtype, group):
    """further: more than 1024 tiles, a workgroup's second tile; nt: one h either side of the 64 MiB (2 h scalars) from which the
    kernel streams with the non-temporal hint -- the last h below it and the first h above it take the element-wise path, the
    threshold itself the vector path.  k1 = 2."""
    item = np.dtype(br.NP[dtype]).itemsize
    hs = cg.sizes(dtype)[group]
    if group == "nt":
        assert [2 * h * item >= br.NT_BYTES for h in hs] == [False, True, True] and hs[1] % br.PACK[dtype] == 0
    for h in hs:
        check_update_exact(ctx, dtype, h, 2, UPDATE_PLACEMENTS[0], seed=9)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_invalid_arguments_launch_nothing(ctx, dtype):
    """h < 0, k1 outside [1, 512], ldv < 2 h with k1 > 1: an error status and nothing written; h = 0 succeeds and writes nothing;
    ldv < 2 h with one column is accepted"""
    T = br.NP[dtype]
    h = 32
    x0 = np.arange(2 * h, dtype=T)
    bx, bv, bc = Buf(ctx, dtype, 2 * h, 0, x0), Buf(ctx, dtype, 4 * h, 0, np.ones(4 * h)), Buf(ctx, dtype, 2 * (cg.KMAX + 1), data=np.ones(2 * (cg.KMAX + 1)))
    for kw in (dict(h=-1), dict(k1=0), dict(k1=-1), dict(k1=cg.KMAX + 1), dict(ldv=2 * h - 1), dict(ldv=-2 * h)):
        a = dict(h=h, k1=2, ldv=2 * h)
        a.update(kw)
        assert ctx.raw(f"ckrylov_update_{dtype}", a["h"], bx.p, bv.p, a["ldv"], a["k1"], bc.p) != 0, kw
    assert ctx.raw(f"cmgs_stage_{dtype}", -1, bx.p, None, None, None, None, None) != 0
    assert ctx.raw(f"ckrylov_update_{dtype}", 0, bx.p, bv.p, 2 * h, 2, bc.p) == 0
    assert ctx.raw(f"cmgs_stage_{dtype}", 0, bx.p, None, None, None, None, None) == 0
    ctx.torch.cuda.synchronize()
    assert same_bits(bx.get(), x0, dtype)
    assert ctx.call(f"ckrylov_update_{dtype}", h, bx.p, bv.p, 0, 1, bc.p) == 0  # y = 1 + i on v = 1 + i: x_r += 0, x_i += 2
    assert same_bits(bx.get(), x0 + np.concatenate([np.zeros(h), np.full(h, 2)]), dtype)
