"""kernels/blas1.hip, entry point by entry point through the C ABI, against tests/blas1_reference.py.

Sizes (N = elements of a 16-byte vector: 2 for f64, 4 for f32 and i32; TILE = 1024 vectors; MAX_PARTIALS = 1024 workgroups):

  small           0, 1, N-1, N, N+1, 256 N - 1
  tile            TILE N - 1, TILE N, TILE N + 1
  ragged          3 TILE N + 5 N + (N-1)                       several tiles, a partial last tile and a scalar tail
  further         N (TILE (MAX_PARTIALS+1) + 300) + (N-1)      a workgroup's second tile: maps, reductions, Gram-Schmidt
  nt              the smallest n of 64 MiB and that n - 1      non-temporal instantiations: maps and reductions

The small, tile and ragged sizes are crossed with element offsets into over-allocated buffers, applied per operand (x aligned
and y not: the scalar path); further and nt run once per family and type, aligned and with one operand off by one element.
Every device buffer has 16 elements of a fixed bit pattern (a NaN) on both sides, compared bitwise on every read-back; output
buffers start as that pattern throughout.

Reductions, single Gram-Schmidt stages and maps on integers are held to the integer result bit for bit (blas1_reference: exact
generators); random floats to a-priori bounds: 4 eps (|a x| + |b y|) for the maps, gamma_d sum |terms| for the coefficients of
the fused Gram-Schmidt chain with d the depth of the schedule, 2 eps (|w| + |h v|) for its updates.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import blas1_reference as br
import oracle

pytestmark = pytest.mark.gpu

GUARD = 16
UINT = {"f64": np.uint64, "f32": np.uint32, "i32": np.uint32}
SINT = {"f64": np.int64, "f32": np.int32, "i32": np.int32}
PATTERN = {"f64": 0x7FF8DEADBEEF0BAD, "f32": 0x7FC0BEEF, "i32": 0x7FC0BEEF}  # quiet NaNs with a payload


def bits(a, dtype):
    return np.ascontiguousarray(a, dtype=br.NP[dtype]).view(UINT[dtype])


def same_bits(a, b, dtype):
    return np.array_equal(bits(a, dtype), bits(b, dtype))


class Ctx:
    def __init__(self, dev):
        import torch

        from cuddhelmholtz_amd import _native as N

        self.torch, self.N, self.lib, self.dev = torch, N, N.lib, dev
        assert self.lib.cuddh_hip_reduce_ws_bytes() == 2 * br.MAX_PARTIALS * 8  # two halves of MAX_PARTIALS doubles

    def call(self, name, *args):
        """cuddh_hip_<name>(*args, stream); a launch error raises"""
        st = C.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        rc = getattr(self.lib, f"cuddh_hip_{name}")(*args, st)
        self.N.check(rc, name)
        return rc


class Buf:
    """n elements of `dtype` at element offset `off` behind a 16-byte boundary, GUARD pattern elements on both sides.
    data None: the n elements are the pattern too (a NaN for the float types)."""

    def __init__(self, ctx, dtype, n, off=0, data=None):
        self.ctx, self.dtype, self.n, self.lo = ctx, dtype, int(n), GUARD + off
        self.item = np.dtype(br.NP[dtype]).itemsize
        self.t = ctx.torch.empty(self.lo + self.n + GUARD, dtype=getattr(ctx.torch, np.dtype(SINT[dtype]).name), device=ctx.dev)
        assert self.t.data_ptr() % 16 == 0 and (GUARD * self.item) % 16 == 0
        self.set(data)

    def set(self, data=None):
        host = np.full(self.lo + self.n + GUARD, PATTERN[self.dtype], dtype=UINT[self.dtype])
        if data is not None:
            assert len(data) == self.n
            host[self.lo:self.lo + self.n] = bits(data, self.dtype)
        self.t.copy_(self.ctx.torch.from_numpy(host.view(SINT[self.dtype])))

    def at(self, k=0):
        return C.c_void_p(self.t.data_ptr() + (self.lo + k) * self.item)

    @property
    def p(self):
        return self.at(0)

    def get(self):
        """the n elements; the guards on both sides are compared bitwise on the way"""
        whole = self.t.cpu().numpy().view(UINT[self.dtype])
        assert np.all(whole[:self.lo] == PATTERN[self.dtype]), "elements before the buffer were written"
        assert np.all(whole[self.lo + self.n:] == PATTERN[self.dtype]), "elements behind the buffer were written"
        return whole[self.lo:self.lo + self.n].view(br.NP[self.dtype]).copy()


@pytest.fixture(scope="module")
def ctx(cuda):
    return Ctx(cuda)


def cases(dtype, groups):
    return [(n, off) for g in groups for n in br.sizes(dtype)[g] for off in br.MAP_OFFSETS[dtype]]


def scalar(dtype, v):
    return float(br.NP[dtype](v)) if dtype != "i32" else int(v)


LARGE = {"further": ("further", 0), "nt_below": ("nt", 0), "nt": ("nt", 1)}
LARGE_OFFSETS = [(0, 0), (0, 1)]


def large_size(dtype, kind):
    g, i = LARGE[kind]
    return br.sizes(dtype)[g][i]


# ================================================================== reductions: dot, sqdist, nrm2
def check_reductions_exact(ctx, dtype, n, offsets, seed):
    rng = np.random.default_rng(seed)
    xmax = 3 if 3 * n <= br.EXACT_LIMIT[dtype] else 1  # (f32 at the non-temporal sizes: |term| <= 1)
    xd, yd = br.exact_dot(n, dtype, rng, xmax)
    xs, ys = br.exact_sqdist(n, dtype, rng)
    xn, k = br.exact_nrm2(n, dtype, rng)
    want = [br.int_dot(xd, yd), br.int_sqdist(xs, ys), k]
    assert br.abs_terms(xd, yd) <= br.EXACT_LIMIT[dtype] and n <= br.EXACT_LIMIT[dtype]
    for ox, oy in offsets:
        ws = Buf(ctx, "f64", 2 * br.MAX_PARTIALS, data=np.zeros(2 * br.MAX_PARTIALS))
        res = Buf(ctx, dtype, 6)
        bx, by = Buf(ctx, dtype, n, ox, xd), Buf(ctx, dtype, n, oy, yd)
        for rep in (0, 1):  # twice: identical bits
            ctx.call(f"dot_{dtype}", n, bx.p, by.p, res.at(rep), ws.p)
        bx.set(xs), by.set(ys)
        for rep in (0, 1):
            ctx.call(f"sqdist_{dtype}", n, bx.p, by.p, res.at(2 + rep), ws.p)
        assert same_bits(bx.get(), xs, dtype) and same_bits(by.get(), ys, dtype)  # inputs and their guards untouched
        bx.set(xn)
        for rep in (0, 1):
            ctx.call(f"nrm2_{dtype}", n, bx.p, res.at(4 + rep), ws.p)
        r = res.get()
        where = f"{dtype} n={n} offsets=({ox},{oy})"
        for i, name in enumerate(("dot", "sqdist", "nrm2")):
            exact = br.NP[dtype](want[i])
            assert int(exact) == want[i]
            assert same_bits(r[2 * i:2 * i + 1], [exact], dtype), f"{name} {where}: {r[2 * i]!r} is not the integer {want[i]}"
            assert same_bits(r[2 * i:2 * i + 1], r[2 * i + 1:2 * i + 2], dtype), f"{name} {where}: two runs differ"
        ws.get()


@pytest.mark.parametrize("group", ["small", "tile", "ragged"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_reductions_equal_the_integer_result(ctx, dtype, group):
    """dot_{f64,f32}, sqdist, nrm2 on exact-integer inputs: a doubled last vector, a dropped tail or a shifted element changes
    the integer; every combination of operand alignments."""
    for n in br.sizes(dtype)[group]:
        check_reductions_exact(ctx, dtype, n, br.MAP_OFFSETS[dtype], seed=n)


@pytest.mark.parametrize("kind", list(LARGE))
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_reductions_equal_the_integer_result_large(ctx, dtype, kind):
    """the second trip of reduce_stage1's tile loop (more than MAX_PARTIALS tiles) and its non-temporal instantiation"""
    check_reductions_exact(ctx, dtype, large_size(dtype, kind), LARGE_OFFSETS, seed=1)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_dot_of_a_vector_with_itself_is_the_two_stream_dot(ctx, dtype):
    """dot(n, x, x) through one pointer reads one stream (MODE 2 of reduce_stage1): the same products, bit for bit, as
    dot(n, x, copy of x), on random floats."""
    s = br.sizes(dtype)
    for n in s["small"] + s["tile"] + s["ragged"] + s["further"] + s["nt"][1:]:
        x = np.random.default_rng(n).standard_normal(n).astype(br.NP[dtype])
        for off in (0, 1) if n < s["further"][0] else (0,):
            ws = Buf(ctx, "f64", 2 * br.MAX_PARTIALS, data=np.zeros(2 * br.MAX_PARTIALS))
            res = Buf(ctx, dtype, 2)
            bx, bc = Buf(ctx, dtype, n, off, x), Buf(ctx, dtype, n, off, x)
            ctx.call(f"dot_{dtype}", n, bx.p, bx.p, res.at(0), ws.p)
            ctx.call(f"dot_{dtype}", n, bx.p, bc.p, res.at(1), ws.p)
            r = res.get()
            assert same_bits(r[:1], r[1:], dtype), f"{dtype} n={n} off={off}: <x,x> {r[0]!r} one stream, {r[1]!r} two streams"
            exact = float(br.dot_wide(x, x, dtype))
            assert abs(float(r[0]) - exact) <= br.reduction_bound(n, dtype, exact)


# ================================================================== maps
def special_values(dtype, n, rng):
    """values for the bitwise maps: random bits of every kind at the marked places"""
    m = br.marked(n, dtype)
    places = [i for k in ("first", "tile_end", "tile2", "last_vector", "tail", "beyond") for i in m[k]]
    if dtype == "i32":
        x = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
        special = [np.iinfo(np.int32).min, np.iinfo(np.int32).max, -1, 0]
    else:
        x = rng.standard_normal(n).astype(br.NP[dtype])
        special = [-0.0, np.inf, -np.inf, np.finfo(br.NP[dtype]).tiny / 4, np.finfo(br.NP[dtype]).max]
    for j, i in enumerate(places):
        x[i] = special[j % len(special)]
    return x


def check_copy_fill(ctx, dtype, n, ox, oy, x):
    where = f"{dtype} n={n} offsets=({ox},{oy})"
    bx, by = Buf(ctx, dtype, n, ox, x), Buf(ctx, dtype, n, oy)  # the destination starts as NaN
    ctx.call(f"copy_{dtype}", n, bx.p, by.p)
    assert same_bits(by.get(), x, dtype), f"copy {where}"
    assert same_bits(bx.get(), x, dtype)
    for value in ([np.iinfo(np.int32).min, -123456789] if dtype == "i32" else [-2.5]):
        by.set(None)
        ctx.call(f"fill_{dtype}", n, scalar(dtype, value), by.p)
        assert np.all(bits(by.get(), dtype) == bits([value], dtype)[0]), f"fill {where}"


@pytest.mark.parametrize("group", ["small", "tile", "ragged"])
@pytest.mark.parametrize("dtype", ["f64", "f32", "i32"])
def test_copy_fill_scal_bitwise(ctx, dtype, group):
    """copy_{f64,f32,i32} and fill_{f64,f32,i32} over NaN-filled destinations (i32: negatives, INT_MIN, INT_MAX), scal_{f64,f32}:
    bitwise, nothing written outside, every combination of operand alignments"""
    for n, (ox, oy) in cases(dtype, [group]):
        rng = np.random.default_rng(n)
        check_copy_fill(ctx, dtype, n, ox, oy, special_values(dtype, n, rng))
        if dtype != "i32" and ox == 0:  # (one operand)
            y = rng.standard_normal(n).astype(br.NP[dtype])
            by = Buf(ctx, dtype, n, oy, y)
            ctx.call(f"scal_{dtype}", n, scalar(dtype, -1.7), by.p)
            assert same_bits(by.get(), y * br.NP[dtype](-1.7), dtype), f"scal {dtype} n={n} offset={oy}"


def check_float_maps(ctx, dtype, n, offsets, seed, full=True):
    rng = np.random.default_rng(seed)
    T, W = br.NP[dtype], br.wide(dtype)
    x, y = rng.standard_normal(n).astype(T), rng.standard_normal(n).astype(T)
    a, b = scalar(dtype, 0.7), scalar(dtype, -1.3)
    tol = br.axpby_bound(a, x, b, y, dtype)
    ref = functools.lru_cache(maxsize=None)(lambda sa: np.asarray(br.axpby_wide(sa * a, x, b, y, dtype)))  # (computed once per case)
    quotient = functools.lru_cache(maxsize=None)(lambda: y.astype(W) / W(a))
    coef = Buf(ctx, dtype, 1, data=[a])

    def close(got, want, bound):
        return bool(np.all(np.abs(got.astype(W) - want) <= bound))

    for ox, oy in offsets:
        where = f"{dtype} n={n} offsets=({ox},{oy})"
        bx, by = Buf(ctx, dtype, n, ox, x), Buf(ctx, dtype, n, oy, y)
        ctx.call(f"axpby_{dtype}", n, a, bx.p, b, by.p)
        assert close(by.get(), ref(1.0), tol), f"axpby {where}"
        assert same_bits(bx.get(), x, dtype)
        # b == 0 must not read y: GMRES does this onto uninitialised basis memory
        by.set(None)
        ctx.call(f"axpby_{dtype}", n, a, bx.p, scalar(dtype, 0.0), by.p)
        assert same_bits(by.get(), T(a) * x, dtype), f"axpby with b == 0 {where}"
        for sa in ((1.0, -1.0) if full else (-1.0,)):  # the coefficient read from device memory
            by.set(y)
            ctx.call(f"axpby_dev_{dtype}", n, sa, coef.p, bx.p, b, by.p)
            assert close(by.get(), ref(sa), tol), f"axpby_dev sa={sa} {where}"
        if ox == 0 or not full:  # (one operand)
            by.set(y)
            ctx.call(f"scal_inv_dev_{dtype}", n, coef.p, by.p)
            assert close(by.get(), quotient(), br.quotient_bound(quotient(), dtype)), f"scal_inv_dev {where}"
            if dtype == "f64" and full:
                by.set(y)
                ctx.call("reciprocal_f64", n, by.p)
                want = W(1) / y.astype(W)
                assert close(by.get(), want, br.quotient_bound(want, dtype)), f"reciprocal {where}"
        assert same_bits(coef.get(), [a], dtype)


@pytest.mark.parametrize("group", ["small", "tile", "ragged"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_axpby_and_scaling_maps(ctx, dtype, group):
    """axpby, axpby_dev_{f64,f32} (sa = +-1), scal_inv_dev_{f64,f32}, reciprocal_f64 on random floats against the wide reference"""
    for n in br.sizes(dtype)[group]:
        check_float_maps(ctx, dtype, n, br.MAP_OFFSETS[dtype], seed=n)


@pytest.mark.parametrize("kind", list(LARGE))
@pytest.mark.parametrize("dtype", ["f64", "f32", "i32"])
def test_maps_large(ctx, dtype, kind):
    """more than MAX_PARTIALS tiles and the non-temporal instantiations of map_kernel: copy and fill of every type, the float
    maps aligned and with y off by one element"""
    n = large_size(dtype, kind)
    x = special_values(dtype, n, np.random.default_rng(2))
    for ox, oy in LARGE_OFFSETS:
        check_copy_fill(ctx, dtype, n, ox, oy, x)
    if dtype != "i32":
        check_float_maps(ctx, dtype, n, LARGE_OFFSETS, seed=3, full=False)


# ================================================================== fused Gram-Schmidt
def stage(ctx, dtype, n, w, vprev, vnext, pin, pout, hout):
    return ctx.call(f"mgs_stage_{dtype}", n, w.p, vprev.p if vprev else None, vnext.p if vnext else None, pin, pout, hout)


def check_mgs_stages_exact(ctx, dtype, n, offs, seed):
    """the four template variants of mgs_stage and mgs_finish on integers: see test_mgs_single_stages_exact"""
    T = br.NP[dtype]
    ow, op, on = offs
    where = f"{dtype} n={n} offsets={offs}"
    w0, p1, p2, dense = br.exact_mgs(n, dtype, np.random.default_rng(seed))
    g, M = br.mgs_grid(n), br.MAX_PARTIALS
    SENT = T(12345.0)
    bw = Buf(ctx, dtype, n, ow, w0)
    bp1, bp2, bd = Buf(ctx, dtype, n, op, p1), Buf(ctx, dtype, n, op, p2), Buf(ctx, dtype, n, on, dense)
    ws = Buf(ctx, dtype, 2 * M, data=np.full(2 * M, SENT))  # the two halves as krylov.cpp lays them out
    hc = Buf(ctx, dtype, 4, data=np.full(4, SENT))
    pa, pb = ws.at(0), ws.at(M)
    state = {"ws": ws.get(), "h": hc.get(), "w": w0}

    def after(half, want_sum, what, w_want=None, h_slot=None, h_want=None):
        """the half written sums to the integer, its slots beyond the workgroups launched and the other half are as they were;
        hout and w are what they must be, bit for bit"""
        got_ws, got_h, got_w = ws.get(), hc.get(), bw.get()
        lo = half * M
        part = got_ws[lo:lo + g]
        assert np.all(part == np.rint(part)), f"{what} {where}: partial sums are not integers"
        assert float(np.sum(part.astype(np.float64))) == float(want_sum), f"{what} {where}: partials sum to {np.sum(part.astype(np.float64))}, not {want_sum}"
        assert same_bits(got_ws[lo + g:lo + M], state["ws"][lo + g:lo + M], dtype), f"{what} {where}: slots beyond workgroup {g} written"
        other = (1 - half) * M
        assert same_bits(got_ws[other:other + M], state["ws"][other:other + M], dtype), f"{what} {where}: the other half of the workspace changed"
        h_expect = state["h"].copy()
        if h_slot is not None:
            h_expect[h_slot] = T(h_want)
            assert int(h_expect[h_slot]) == h_want
        assert same_bits(got_h, h_expect, dtype), f"{what} {where}: hout {got_h} expected {h_expect}"
        w_expect = state["w"] if w_want is None else w_want
        assert np.array_equal(got_w, w_expect), f"{what} {where}: w differs at {np.flatnonzero(got_w != w_expect)[:8]}"
        state.update(ws=got_ws, h=got_h, w=w_expect)

    # <false, true>: partial sums of <w, p1>, w untouched, hout untouched
    stage(ctx, dtype, n, bw, None, bp1, pa, pa, hc.at(0))
    h1 = br.int_dot(w0, p1)
    after(0, h1, "first stage")
    # <true, true>: h = <w, p1>, w -= h p1, partial sums of <w, dense>
    stage(ctx, dtype, n, bw, bp1, bd, pa, pb, hc.at(0))
    w1 = w0 - T(h1) * p1
    after(1, br.int_dot(w1, dense), "stage with both vectors", w_want=w1, h_slot=0, h_want=h1)
    # <false, true> again, into the half that was read
    stage(ctx, dtype, n, bw, None, bp2, pa, pa, hc.at(1))
    h2 = br.int_dot(w1, p2)
    after(0, h2, "second first stage")
    # <true, false>: the sum is observed through hout, then partial sums of <w, w>
    stage(ctx, dtype, n, bw, bp2, None, pa, pb, hc.at(1))
    w2 = w1 - T(h2) * p2
    ww = br.int_dot(w2, w2)
    assert br.abs_terms(w2) <= br.EXACT_LIMIT[dtype]
    after(1, ww, "last projection stage", w_want=w2, h_slot=1, h_want=h2)
    # <false, false>: <w, w> again, nothing else moves
    stage(ctx, dtype, n, bw, None, None, pb, pa, hc.at(2))
    after(0, ww, "norm-only stage")
    for b, v in ((bp1, p1), (bp2, p2), (bd, dense)):
        assert same_bits(b.get(), v, dtype)
    # finish on partials that sum to 16: the norm is 4, every element is divided once, exactly
    part = np.full(2 * M, SENT)
    part[M:M + g] = 0
    part[M] = 16
    ws.set(part)
    ctx.call(f"mgs_finish_{dtype}", n, bw.p, pb, hc.at(3))
    got_h = hc.get()
    assert same_bits(got_h[3:], [T(4)], dtype) and same_bits(got_h[:3], state["h"][:3], dtype), f"finish {where}: hout {got_h}"
    assert same_bits(bw.get(), w2 / T(4), dtype), f"finish {where}: w is not w / 4"
    assert same_bits(ws.get(), part, dtype)
    # finish on the partial sums of <w, w>: the norm is the correctly rounded root of the integer
    if ww > 0:
        bw.set(w2)
        stage(ctx, dtype, n, bw, None, None, pb, pa, hc.at(2))
        ctx.call(f"mgs_finish_{dtype}", n, bw.p, pa, hc.at(3))
        nrm = hc.get()[3]
        assert same_bits([nrm], [np.sqrt(T(ww))], dtype), f"finish {where}: norm {nrm!r}, <w,w> = {ww}"
        W = br.wide(dtype)
        want = w2.astype(W) / W(nrm)
        assert np.all(np.abs(bw.get().astype(W) - want) <= br.quotient_bound(want, dtype)), f"finish {where}: w / norm"


@pytest.mark.parametrize("group", ["small", "tile", "ragged"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mgs_single_stages_exact(ctx, dtype, group):
    """mgs_stage_{f64,f32} in its four variants and mgs_finish_{f64,f32} on exact-integer inputs (w in {-2..2}, sparse +-1
    vectors at the first element, the tile boundary, the last full vector and the tail, a dense +-1 vector): a stage without
    v_prev produces the partial sums, the next one consumes them.  Bitwise: *hout is the integer <w, v_prev>, every element of the new
    w is w - h v_prev, the new partials sum to <w, v_next> (or <w, w>), the other half of the workspace and the slots beyond the
    workgroups launched are unchanged, w is unchanged by a stage without v_prev."""
    for n in br.sizes(dtype)[group]:
        for offs in br.MGS_OFFSETS:
            check_mgs_stages_exact(ctx, dtype, n, offs, seed=n)


@pytest.mark.parametrize("offs", [(0, 0, 0), (0, 1, 0)])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mgs_single_stages_exact_further_tiles(ctx, dtype, offs):
    """more than MAX_PARTIALS tiles: the 'further tiles' loops of mgs_stage_kernel and mgs_finish_kernel, with a nonzero of the
    sparse vectors beyond tile 1024"""
    (n,) = br.sizes(dtype)["further"]
    assert br.marked(n, dtype)["beyond"]
    check_mgs_stages_exact(ctx, dtype, n, offs, seed=5)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mgs_finish_with_zero_partials(ctx, dtype):
    """a breakdown: the norm is exactly 0.0 and the call succeeds (w becomes non-finite by design: nothing is asserted about it)"""
    T = br.NP[dtype]
    for n in (br.sizes(dtype)["tile"][2], br.sizes(dtype)["ragged"][0]):
        bw = Buf(ctx, dtype, n, 0, np.random.default_rng(n).standard_normal(n).astype(T))
        ws = Buf(ctx, dtype, 2 * br.MAX_PARTIALS, data=np.zeros(2 * br.MAX_PARTIALS))
        hc = Buf(ctx, dtype, 2)
        assert ctx.call(f"mgs_finish_{dtype}", n, bw.p, ws.p, hc.at(0)) == 0
        assert same_bits(hc.get()[:1], [T(0.0)], dtype)
        bw.get(), ws.get()  # (guards)


@functools.lru_cache(maxsize=None)
def chain_inputs(dtype, n):
    rng = np.random.default_rng(11)
    V = br.orthonormal_columns(n, 3, rng, dtype)
    return V, rng.standard_normal(n).astype(br.NP[dtype])


def check_projection(dtype, n, what, w_before, v, h, w_after):
    """one projection step as the device did it: its coefficient against the inner product of its own w, its update against
    w - h v with the h it reported"""
    W = br.wide(dtype)
    ref = br.dot_wide(w_before, v, dtype)
    tol = br.reduction_bound(n, dtype, br.abs_dot(w_before, v))
    assert abs(W(h) - ref) <= tol, f"{what}: h = {h!r}, <w, v> = {ref!r}, bound {tol:.3e}"
    upd = w_before.astype(W) - W(h) * v.astype(W)
    err = np.abs(w_after.astype(W) - upd)
    bound = br.projection_bound(w_before, h, v, dtype)
    assert np.all(err <= bound), f"{what}: update off at {np.flatnonzero(err > bound)[:8]}"
    return tol


def check_normalised(dtype, n, what, V, w_before, nrm, w_after):
    W = br.wide(dtype)
    true = float(np.sqrt(br.dot_wide(w_before, w_before, dtype)))
    assert abs(float(nrm) - true) <= br.norm_bound(n, dtype, true), f"{what}: norm {nrm!r} vs {true!r}"
    want = w_before.astype(W) / W(nrm)
    assert np.all(np.abs(w_after.astype(W) - want) <= br.quotient_bound(want, dtype)), f"{what}: w / norm"
    assert abs(float(br.dot_wide(w_after, w_after, dtype)) - 1) <= br.unit_norm_bound(n, dtype), f"{what}: not of unit norm"
    loss = max(abs(float(br.dot_wide(w_after, v, dtype))) for v in V)
    assert loss <= br.orthogonality_bound(dtype), f"{what}: |<w, v_j>| = {loss:.3e}"
    return true


def check_mgs_chain(ctx, dtype, n, offs):
    T = br.NP[dtype]
    V, w0 = chain_inputs(dtype, n)
    ow, op, on = offs
    M = br.MAX_PARTIALS
    where = f"{dtype} n={n} offsets={offs}"
    bv = [Buf(ctx, dtype, n, o, v) for o, v in zip((op, on, op), V)]
    # ---- fused: what krylov.cpp::queue_step queues for k = 2
    bw = Buf(ctx, dtype, n, ow, w0)
    ws = Buf(ctx, dtype, 2 * M, data=np.zeros(2 * M))
    hc = Buf(ctx, dtype, 4, data=np.zeros(4))
    pa, pb = ws.at(0), ws.at(M)
    stage(ctx, dtype, n, bw, None, bv[0], pa, pa, hc.at(0))
    wf = [bw.get()]
    assert same_bits(wf[0], w0, dtype)
    for j in range(3):
        stage(ctx, dtype, n, bw, bv[j], bv[j + 1] if j < 2 else None, pa, pb, hc.at(j))
        pa, pb = pb, pa
        wf.append(bw.get())
    ctx.call(f"mgs_finish_{dtype}", n, bw.p, pa, hc.at(3))
    hf, w_fused = hc.get(), bw.get()
    tol_f = [check_projection(dtype, n, f"fused stage {j} {where}", wf[j], V[j], hf[j], wf[j + 1]) for j in range(3)]
    check_normalised(dtype, n, f"fused finish {where}", V, wf[3], hf[3], w_fused)
    # ---- unfused: dot + axpby_dev per basis vector, as the sharded GMRES does it
    bw.set(w0)
    wsd = Buf(ctx, "f64", 2 * M, data=np.zeros(2 * M))
    hu_b = Buf(ctx, dtype, 4, data=np.zeros(4))
    wu = [w0]
    for j in range(3):
        ctx.call(f"dot_{dtype}", n, bw.p, bv[j].p, hu_b.at(j), wsd.p)
        ctx.call(f"axpby_dev_{dtype}", n, scalar(dtype, -1.0), hu_b.at(j), bv[j].p, scalar(dtype, 1.0), bw.p)
        wu.append(bw.get())
    ctx.call(f"nrm2_{dtype}", n, bw.p, hu_b.at(3), wsd.p)
    ctx.call(f"scal_inv_dev_{dtype}", n, hu_b.at(3), bw.p)
    hu, w_unfused = hu_b.get(), bw.get()
    tol_u = [check_projection(dtype, n, f"unfused step {j} {where}", wu[j], V[j], hu[j], wu[j + 1]) for j in range(3)]
    check_normalised(dtype, n, f"unfused normalisation {where}", V, wu[3], hu[3], w_unfused)
    # ---- the two against each other: each coefficient is within its bound of the inner product of its own w, and the two w differ
    # by what the steps before let them differ
    for j in range(3):
        dw = wf[j].astype(np.float64) - wu[j].astype(np.float64)
        assert abs(float(hf[j]) - float(hu[j])) <= tol_f[j] + tol_u[j] + br.abs_dot(dw, V[j]), f"h[{j}] fused {hf[j]!r} unfused {hu[j]!r} {where}"
    dw = float(np.linalg.norm(wf[3].astype(np.float64) - wu[3].astype(np.float64)))
    true = float(np.sqrt(br.dot_wide(wf[3], wf[3], dtype)))
    assert abs(float(hf[3]) - float(hu[3])) <= 2 * br.norm_bound(n, dtype, true + dw) + dw, f"norm fused {hf[3]!r} unfused {hu[3]!r} {where}"
    for b, v in zip(bv, V):
        assert same_bits(b.get(), v, dtype)


@pytest.mark.parametrize("offs", br.MGS_OFFSETS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mgs_chain_on_random_floats(ctx, dtype, offs):
    """The chain krylov.cpp::queue_step issues for k = 2 (first stage, three projection stages on orthonormal v0..v2, finish) on a
    standard normal w: every hout[j] against the inner product of the device's own w before that stage (gamma_d sum |terms|, d from
    the schedule: blas1_reference.reduction_depth), every update elementwise against w - hout[j] v_j (2 eps (|w| + |h v|): workgroups
    that disagree on h fail here), hout[3] the norm and the result of unit norm, |<w, v_j>| <= 1 eps (the reference chain in the kernel's
    precision loses 0.146 eps in f64 and 0.041 eps in f32: blas1_reference.ORTHOGONALITY_EPS), and the unfused dot + axpby_dev
    sequence on the same inputs within the same bounds."""
    check_mgs_chain(ctx, dtype, br.sizes(dtype)["ragged"][0], offs)


@pytest.mark.parametrize("offs", [(0, 0, 0), (0, 1, 0)])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mgs_chain_on_random_floats_further_tiles(ctx, dtype, offs):
    check_mgs_chain(ctx, dtype, br.sizes(dtype)["further"][0], offs)


# ================================================================== indexed and exchange kernels
@pytest.mark.parametrize("n", br.INDEXED_SIZES)
def test_gather_scatter_add_zero_indexed(ctx, n):
    """gather_f64 through a projection with repeats, scatter_add_f64 and zero_indexed_f64 through an injective one (their
    precondition): touched entries bitwise, every other entry bit-identical; the last size takes the grid-stride loops round again"""
    rng = np.random.default_rng(n)
    nvec = 2 * n + 7
    x_long, x_short, y0 = rng.standard_normal(nvec), rng.standard_normal(n), rng.standard_normal(nvec)
    proj = rng.integers(0, nvec, n)
    if n > 0:
        proj[0], proj[-1] = nvec - 1, (0 if n > 1 else nvec - 1)
    if n > 2:
        proj[1] = proj[2] = proj[0]  # repeats
    bp = Buf(ctx, "i32", n, data=proj.astype(np.int32))
    bx, by = Buf(ctx, "f64", nvec, data=x_long), Buf(ctx, "f64", n)
    assert ctx.call("gather_f64", n, bp.p, bx.p, by.p) == 0
    assert same_bits(by.get(), x_long[proj], "f64") and same_bits(bx.get(), x_long, "f64")
    inj = rng.permutation(nvec)[:n]
    bp.set(inj.astype(np.int32))
    bx, by = Buf(ctx, "f64", n, data=x_short), Buf(ctx, "f64", nvec, data=y0)
    assert ctx.call("scatter_add_f64", n, bp.p, bx.p, by.p) == 0
    want = y0.copy()
    want[inj] = y0[inj] + x_short
    assert same_bits(by.get(), want, "f64")
    assert ctx.call("zero_indexed_f64", n, bp.p, by.p) == 0
    want[inj] = 0.0
    assert same_bits(by.get(), want, "f64")
    assert same_bits(bp.get(), inj.astype(np.int32), "i32") and same_bits(bx.get(), x_short, "f64")


@pytest.mark.parametrize("n", br.INDEXED_SIZES)
def test_csr_sum_adds_in_the_listed_order(ctx, n):
    """csr_sum_f64, rows of length 0, 1, 2, 7 and 64 over entries that include 1e16, 1 and -1e16: bitwise the strictly left-to-right
    float64 sum; accumulate = 0 overwrites (0.0 on empty rows), accumulate = 1 starts from y and leaves empty rows alone; two runs agree"""
    rng = np.random.default_rng(n + 1)
    off, src, x = br.csr_case(n, 2 * n + 7, rng)
    y0 = rng.standard_normal(n)
    boff, bsrc, bx = Buf(ctx, "i32", n + 1, data=off), Buf(ctx, "i32", len(src), data=src), Buf(ctx, "f64", len(x), data=x)
    runs = []
    for _ in range(2):
        by = Buf(ctx, "f64", n, data=np.full(n, 7.5))
        assert ctx.call("csr_sum_f64", n, boff.p, bsrc.p, bx.p, by.p, 0) == 0
        runs.append(by.get())
    want = br.csr_sum_ref(off, src, x, None, False)
    assert same_bits(runs[0], want, "f64") and same_bits(runs[0], runs[1], "f64")
    empty = np.flatnonzero(np.diff(off) == 0)
    assert np.all(bits(runs[0][empty], "f64") == 0)
    by = Buf(ctx, "f64", n, data=y0)
    assert ctx.call("csr_sum_f64", n, boff.p, bsrc.p, bx.p, by.p, 1) == 0
    got = by.get()
    assert same_bits(got, br.csr_sum_ref(off, src, x, y0, True), "f64") and same_bits(got[empty], y0[empty], "f64")
    for b, v, t in ((boff, off, "i32"), (bsrc, src, "i32"), (bx, x, "f64")):
        assert same_bits(b.get(), v, t)


@pytest.mark.parametrize("n", br.INDEXED_SIZES)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_trace_pack_unpack(ctx, dtype, n):
    """trace_pack_{f32,f64} / trace_unpack_{f32,f64}: slot t stands for entries t and n_half + t, packed as buf[i] | buf[n + i];
    clear = 0 leaves v intact, clear = 1 zeroes exactly the two entries per slot; pack then unpack restores v; nothing else moves"""
    rng = np.random.default_rng(n + 2)
    n_half = 2 * n + 7
    v = rng.standard_normal(2 * n_half).astype(br.NP[dtype])
    slot = rng.permutation(n_half)[:n]
    bs, bv, bb = Buf(ctx, "i32", n, data=slot.astype(np.int32)), Buf(ctx, dtype, 2 * n_half, data=v), Buf(ctx, dtype, 2 * n)
    packed = np.concatenate([v[slot], v[n_half + slot]])
    assert ctx.call(f"trace_pack_{dtype}", n, n_half, bs.p, bv.p, bb.p, 0) == 0
    assert same_bits(bb.get(), packed, dtype) and same_bits(bv.get(), v, dtype)
    bb.set(None)
    assert ctx.call(f"trace_pack_{dtype}", n, n_half, bs.p, bv.p, bb.p, 1) == 0
    cleared = v.copy()
    cleared[slot] = 0
    cleared[n_half + slot] = 0
    assert same_bits(bb.get(), packed, dtype) and same_bits(bv.get(), cleared, dtype)
    assert ctx.call(f"trace_unpack_{dtype}", n, n_half, bs.p, bb.p, bv.p) == 0
    assert same_bits(bv.get(), v, dtype) and same_bits(bb.get(), packed, dtype)
    assert same_bits(bs.get(), slot.astype(np.int32), "i32")


@pytest.mark.parametrize("n", br.INDEXED_SIZES)
def test_halo_pack_unpack(ctx, n):
    """halo_pack_f64 / halo_unpack_f64: entries t and n_half + t travel as the pair (buf[2 i], buf[2 i + 1]); clear as for the trace
    kernels; add = 0 overwrites, add = 1 adds (bitwise the float64 v + b); one pack serves several contiguous pieces, unpacked
    one launch per piece with ids and buf offset as dist.py offsets them"""
    rng = np.random.default_rng(n + 3)
    n_half = 2 * n + 7
    v, other = rng.standard_normal(2 * n_half), rng.standard_normal(2 * n_half)
    ids = rng.permutation(n_half)[:n]
    bi, bv, bb = Buf(ctx, "i32", n, data=ids.astype(np.int32)), Buf(ctx, "f64", 2 * n_half, data=v), Buf(ctx, "f64", 2 * n)
    packed = np.stack([v[ids], v[n_half + ids]], axis=1).reshape(-1)
    assert ctx.call("halo_pack_f64", n, n_half, bi.p, bv.p, bb.p, 0) == 0
    assert same_bits(bb.get(), packed, "f64") and same_bits(bv.get(), v, "f64")
    bb.set(None)
    assert ctx.call("halo_pack_f64", n, n_half, bi.p, bv.p, bb.p, 1) == 0
    cleared = v.copy()
    cleared[ids] = 0
    cleared[n_half + ids] = 0
    assert same_bits(bb.get(), packed, "f64") and same_bits(bv.get(), cleared, "f64")
    # add = 0 overwrites whatever is there
    bo = Buf(ctx, "f64", 2 * n_half, data=other)
    assert ctx.call("halo_unpack_f64", n, n_half, bi.p, bb.p, bo.p, 0) == 0
    want = other.copy()
    want[ids], want[n_half + ids] = v[ids], v[n_half + ids]
    assert same_bits(bo.get(), want, "f64")
    # add = 1, piece by piece
    bo.set(other)
    pieces = [n // 3, n // 3, n - 2 * (n // 3)]
    o = 0
    for k in pieces:
        assert ctx.call("halo_unpack_f64", k, n_half, bi.at(o), bb.at(2 * o), bo.p, 1) == 0
        o += k
        want = other.copy()
        want[ids[:o]] = other[ids[:o]] + v[ids[:o]]
        want[n_half + ids[:o]] = other[n_half + ids[:o]] + v[n_half + ids[:o]]
        assert same_bits(bo.get(), want, "f64"), f"after {o} of {n} ids"
    assert same_bits(bb.get(), packed, "f64") and same_bits(bi.get(), ids.astype(np.int32), "i32")


@pytest.mark.parametrize("n", br.INDEXED_SIZES)
def test_diag_scale(ctx, n):
    """diag_scale_f64: accumulate = 0 is bitwise (c p) x, also with x aliasing y (DiagInvMassMatrix in place); accumulate = 1 within
    2 eps (|y| + |v|) (the build contracts the sum into a fused multiply-add)"""
    rng = np.random.default_rng(n + 4)
    c = -0.7
    p, x, y0 = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    bp, bx, by = Buf(ctx, "f64", n, data=p), Buf(ctx, "f64", n, data=x), Buf(ctx, "f64", n)
    assert ctx.call("diag_scale_f64", n, 0, c, bp.p, bx.p, by.p) == 0
    assert same_bits(by.get(), (c * p) * x, "f64")
    by.set(y0)
    assert ctx.call("diag_scale_f64", n, 1, c, bp.p, bx.p, by.p) == 0
    vl = (c * p).astype(np.longdouble) * x.astype(np.longdouble)
    err = np.abs(by.get().astype(np.longdouble) - (y0.astype(np.longdouble) + vl))
    assert np.all(err <= 2 * np.finfo(np.float64).eps * (np.abs(y0) + np.abs(np.asarray(vl, dtype=np.float64))))
    by.set(y0)
    assert ctx.call("diag_scale_f64", n, 0, c, bp.p, by.p, by.p) == 0  # in place
    assert same_bits(by.get(), (c * p) * y0, "f64")
    assert same_bits(bp.get(), p, "f64") and same_bits(bx.get(), x, "f64")


# ================================================================== every entry point of the layer has a test above
COVERED_BY = {
    "mgs_stage_f64": "test_mgs_single_stages_exact", "mgs_stage_f32": "test_mgs_single_stages_exact",
    "mgs_finish_f64": "test_mgs_single_stages_exact", "mgs_finish_f32": "test_mgs_single_stages_exact",
    "axpby_dev_f64": "test_axpby_and_scaling_maps", "axpby_dev_f32": "test_axpby_and_scaling_maps",
    "scal_inv_dev_f64": "test_axpby_and_scaling_maps", "scal_inv_dev_f32": "test_axpby_and_scaling_maps",
    "copy_i32": "test_copy_fill_scal_bitwise", "fill_i32": "test_copy_fill_scal_bitwise",
    "diag_scale_f64": "test_diag_scale", "reciprocal_f64": "test_axpby_and_scaling_maps",
    "gather_f64": "test_gather_scatter_add_zero_indexed", "scatter_add_f64": "test_gather_scatter_add_zero_indexed",
    "zero_indexed_f64": "test_gather_scatter_add_zero_indexed", "csr_sum_f64": "test_csr_sum_adds_in_the_listed_order",
    "trace_pack_f32": "test_trace_pack_unpack", "trace_pack_f64": "test_trace_pack_unpack",
    "trace_unpack_f32": "test_trace_pack_unpack", "trace_unpack_f64": "test_trace_pack_unpack",
    "halo_pack_f64": "test_halo_pack_unpack", "halo_unpack_f64": "test_halo_pack_unpack",
}


def test_every_entry_point_is_exported_and_has_a_test(ctx):
    import inspect
    import sys

    assert len(COVERED_BY) == 22
    for name, test in COVERED_BY.items():
        assert hasattr(ctx.lib, f"cuddh_hip_{name}"), name
        text = "".join(inspect.getsource(f) for f in (globals()[test], stage, check_mgs_stages_exact, check_float_maps, check_copy_fill))
        stem = name.rsplit("_", 1)[0]
        assert f'"{name}"' in text or f'"{stem}_{{dtype}}"' in text, f"{test} does not call {name}"
    assert sys.modules[__name__].pytestmark.name == "gpu"


# ================================================================== GMRES breakdown (callback path)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_gmres_breakdown_through_the_callback_path(ctx, dtype):
    """A = identity, b = e_1, x_0 = 0: h[1] == 0 exactly, the fresh basis vector is 0 / 0 and must never be used"""
    import cuddhelmholtz_amd as cd

    torch = ctx.torch
    n, T = 37, br.NP[dtype]
    bh = np.zeros(n, dtype=T)
    bh[0] = 1
    b = torch.from_numpy(bh).to(ctx.dev)
    x = torch.zeros_like(b)
    out = cd.gmres(n, x, lambda u, v: v.copy_(u), b, 5, 10, 1e-6)
    xo, info = oracle.gmres(lambda u: u.copy(), bh, m=5, maxit=10, tol=1e-6, dtype=T)
    got = x.cpu().numpy()
    assert out.success and info["success"]
    assert np.all(np.isfinite(got)) and same_bits(got, bh, dtype) and same_bits(xo, bh, dtype)
    assert out.num_matvec == info["num_matvec"] == 3
    assert list(out.res_norm) == list(info["res_norm"]) == [1.0, 0.0]
