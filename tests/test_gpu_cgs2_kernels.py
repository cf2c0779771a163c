"""cgs_pass_{f64,f32} and cgs_reduce_{f64,f32} of kernels/blas1.hip through the C ABI, against tests/cgs2_reference.py.

A partial-sum buffer has rows of ROW = 1024 scalars: workgroup b of the g = mgs_grid(n) launched writes <w, w> to [b] and
<w, v_j> to [(1 + j) ROW + b].  Sizes as in test_gpu_blas1_kernels.py (N = elements of a 16-byte vector, TILE = 1024 vectors):

  small     0, 1, N-1, N, N+1, 256 N - 1        tile   TILE N - 1, TILE N, TILE N + 1
  ragged    3 TILE N + 5 N + (N-1)              several tiles, a partial last tile and a scalar tail
  further   N (TILE 1025 + 300) + (N-1)         a workgroup's second tile (k1 = 3: about 50 MB of basis)

crossed with k1 in {1, 2, KC, KC + 1, 2 KC + 1} (KC = 4 basis vectors per register chunk; 33 at the ragged size) and with the
placements: everything aligned with ldv a multiple of N; w off by one element; V off by one element; ldv = n (unaligned basis
vectors when n is no multiple of N); ldv with ldv mod N = 1 (every second basis vector unaligned in f64): the last four
must take the element-wise path for ALL vectors and still match.  Integer inputs whose sums stay below the exactness limit: every
summation order gives the same bits, so the comparison is bitwise.  Buffers carry NaN guards on both sides (compared on every
read-back), the gaps between basis vectors hold a value that would change every sum, outputs start as a sentinel.
"""
import ctypes as C

import numpy as np
import pytest

import blas1_reference as br
import cgs2_reference as cr

pytestmark = pytest.mark.gpu

GUARD = 16
UINT = {"f64": np.uint64, "f32": np.uint32}
SINT = {"f64": np.int64, "f32": np.int32}
PATTERN = {"f64": 0x7FF8DEADBEEF0BAD, "f32": 0x7FC0BEEF}  # quiet NaNs with a payload
SENT = 12345.0  # initial value of outputs
GAP = 999.0  # between basis vectors
ROW = cr.ROW
PLACEMENTS = [(0, 0, "padded"), (1, 0, "padded"), (0, 1, "padded"), (0, 0, "tight"), (0, 0, "odd")]  # (w offset, V offset, ldv)
K1S = (1, 2, cr.KC, cr.KC + 1, 2 * cr.KC + 1)


def bits(a, dtype):
    return np.ascontiguousarray(a, dtype=br.NP[dtype]).view(UINT[dtype])


def same_bits(a, b, dtype):
    return np.array_equal(bits(a, dtype), bits(b, dtype))


class Ctx:
    def __init__(self, dev):
        import torch

        from cuddhelmholtz_amd import _native as N

        self.torch, self.N, self.lib, self.dev = torch, N, N.lib, dev

    def raw(self, name, *args):
        """cuddh_hip_<name>(*args, stream): the status"""
        st = C.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        return getattr(self.lib, f"cuddh_hip_{name}")(*args, st)

    def call(self, name, *args):
        """the same; a launch error raises"""
        rc = self.raw(name, *args)
        self.N.check(rc, name)
        return rc


class Buf:
    """n elements of `dtype` at element offset `off` behind a 16-byte boundary, GUARD pattern elements on both sides"""

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
        whole = self.t.cpu().numpy().view(UINT[self.dtype])
        assert np.all(whole[:self.lo] == PATTERN[self.dtype]), "elements before the buffer were written"
        assert np.all(whole[self.lo + self.n:] == PATTERN[self.dtype]), "elements behind the buffer were written"
        return whole[self.lo:self.lo + self.n].view(br.NP[self.dtype]).copy()


@pytest.fixture(scope="module")
def ctx(cuda):
    return Ctx(cuda)


def cgs_pass(ctx, dtype, n, w, V, ldv, k1, update, dots, cin, ncin, cstride, hacc, hout, pout, raw=False):
    f = ctx.raw if raw else ctx.call
    return f(f"cgs_pass_{dtype}", n, w, V, ldv, k1, update, dots, cin, ncin, cstride, hacc, hout, pout)


def leading_dimension(n, dtype, mode):
    N = br.PACK[dtype]
    padded = -(-max(n, 1) // N) * N
    return {"padded": padded, "tight": max(n, 1), "odd": padded + 1}[mode]


def basis_array(V, n, ldv, dtype):
    """the k1 vectors ldv apart (the last one n long), GAP between them"""
    k1 = len(V)
    flat = np.full(ldv * (k1 - 1) + n, GAP, dtype=br.NP[dtype])
    for j, v in enumerate(V):
        flat[j * ldv:j * ldv + n] = v
    return flat


def check_rows(got, before, g, k1, want, what):
    """rows 0..len(want)-1 of a partial buffer: the first g slots are integers that sum to want[row], everything else is as before"""
    expect = before.copy()
    for r, total in enumerate(want):
        part = got[r * ROW:r * ROW + g]
        assert np.all(part == np.rint(part)), f"{what}: row {r} holds non-integers"
        assert float(np.sum(part.astype(np.float64))) == float(total), f"{what}: row {r} sums to {np.sum(part.astype(np.float64))}, not {total}"
        expect[r * ROW:r * ROW + g] = part
    assert np.array_equal(got.view(np.uint8), expect.view(np.uint8)), f"{what}: slots outside the {g} workgroups' or other rows were written"


def check_cgs_exact(ctx, dtype, n, k1, placement, seed):
    T = br.NP[dtype]
    ow, ov, mode = placement
    ldv = leading_dimension(n, dtype, mode)
    where = f"{dtype} n={n} k1={k1} placement={placement} ldv={ldv}"
    w0, V = cr.exact_cgs(n, dtype, k1, np.random.default_rng(seed))
    e = cr.exact_step(w0, V)
    assert e["largest"] <= br.EXACT_LIMIT[dtype]
    h_ref, q_ref, c1_ref = cr.cgs_step_ref(w0, V, dtype=dtype) if e["wwC"] > 0 else (None, None, None)
    if h_ref is not None:  # the named reference and the integer restatement are the same numbers
        assert np.array_equal(h_ref[:k1], e["h"]) and np.array_equal(c1_ref, e["dA"]) and float(h_ref[k1]) ** 2 == pytest.approx(e["wwC"], rel=1e-12)
    g = br.mgs_grid(n)
    flat = basis_array(V, n, ldv, dtype)
    bw, bw2, bv = Buf(ctx, dtype, n, ow, w0), Buf(ctx, dtype, n, ow, w0), Buf(ctx, dtype, len(flat), ov, flat)
    rows = (k1 + 1) * ROW
    pa, pb, pb2 = (Buf(ctx, dtype, rows, data=np.full(rows, SENT)) for _ in range(3))
    hc1, hc1b, hcol, hcolb, redA, redB = (Buf(ctx, dtype, k1 + 2, data=np.full(k1 + 2, SENT)) for _ in range(6))
    sent = np.full(rows, T(SENT))

    def column(values):
        out = np.full(k1 + 2, T(SENT))
        out[:len(values)] = np.asarray(values, dtype=T)
        assert np.array_equal(out[:len(values)].astype(np.int64), np.asarray(values, dtype=np.int64))
        return out

    # ---- pass A: dots only
    assert cgs_pass(ctx, dtype, n, bw.p, bv.p, ldv, k1, 0, 1, None, 0, 0, None, None, pa.p) == 0
    gotA = pa.get()
    check_rows(gotA, sent, g, k1, [e["wwA"], *e["dA"]], f"pass A {where}")
    assert same_bits(bw.get(), w0, dtype), f"pass A {where}: w changed"
    # ---- cgs_reduce against the integer sums
    ctx.call(f"cgs_reduce_{dtype}", n, k1, pa.p, redA.p)
    assert same_bits(redA.get(), column([*e["dA"], e["wwA"]]), dtype), f"reduce of pass A {where}: {redA.get()}"
    # ---- pass B: update with the sums of pass A's partials, dots of the updated w
    assert cgs_pass(ctx, dtype, n, bw.p, bv.p, ldv, k1, 1, 1, pa.at(ROW), g, ROW, None, hc1.p, pb.p) == 0
    gotB = pb.get()
    check_rows(gotB, sent, g, k1, [e["wwB"], *e["dB"]], f"pass B {where}")
    assert same_bits(hc1.get(), column(e["dA"]), dtype), f"pass B {where}: hout {hc1.get()}"
    w1 = bw.get()
    assert np.array_equal(w1, e["wB"].astype(T)), f"pass B {where}: w differs at {np.flatnonzero(w1 != e['wB'])[:8]}"
    assert same_bits(pa.get(), gotA, dtype), f"pass B {where}: its input partials changed"
    # ---- the same pass in the ncin = 1 form (coefficients already final): identical w, hout and partials
    assert cgs_pass(ctx, dtype, n, bw2.p, bv.p, ldv, k1, 1, 1, redA.p, 1, 1, None, hc1b.p, pb2.p) == 0
    assert same_bits(bw2.get(), w1, dtype) and same_bits(hc1b.get(), hc1.get(), dtype) and same_bits(pb2.get(), gotB, dtype), f"ncin = 1 form {where}"
    ctx.call(f"cgs_reduce_{dtype}", n, k1, pb.p, redB.p)
    assert same_bits(redB.get(), column([*e["dB"], e["wwB"]]), dtype), f"reduce of pass B {where}"
    # ---- pass C: update with pass B's sums, hout = hacc + c, <w, w> only (into the buffer pass A wrote: its other rows stay)
    assert cgs_pass(ctx, dtype, n, bw.p, bv.p, ldv, k1, 1, 2, pb.at(ROW), g, ROW, hc1.p, hcol.p, pa.p) == 0
    gotC = pa.get()
    check_rows(gotC, gotA, g, k1, [e["wwC"]], f"pass C {where}")
    assert same_bits(hcol.get(), column(e["h"]), dtype), f"pass C {where}: hout {hcol.get()} expected {e['h']}"
    w2 = bw.get()
    assert np.array_equal(w2, e["wC"].astype(T)), f"pass C {where}: w differs at {np.flatnonzero(w2 != e['wC'])[:8]}"
    # (pass C through final coefficients, hacc given: the partitioned path's form)
    assert cgs_pass(ctx, dtype, n, bw2.p, bv.p, ldv, k1, 1, 2, redB.p, 1, 1, hc1b.p, hcolb.p, pb2.p) == 0
    assert same_bits(bw2.get(), w2, dtype) and same_bits(hcolb.get(), hcol.get(), dtype), f"pass C, ncin = 1 form {where}"
    # ---- the existing finish kernel reads row 0
    if e["wwC"] > 0:
        ctx.call(f"mgs_finish_{dtype}", n, bw.p, pa.p, hcol.at(k1))
        hc = hcol.get()
        assert same_bits(hc[k1:k1 + 1], [np.sqrt(T(e["wwC"]))], dtype) and same_bits(hc[:k1], column(e["h"])[:k1], dtype), f"finish {where}: {hc}"
        assert same_bits(hc[k1 + 1:], [T(SENT)], dtype)
        W = br.wide(dtype)
        want = w2.astype(W) / W(hc[k1])
        assert np.all(np.abs(bw.get().astype(W) - want) <= br.quotient_bound(want, dtype)), f"finish {where}: w / norm"
        assert np.all(np.abs(bw.get().astype(W) - q_ref) <= 2 * np.asarray(br.quotient_bound(q_ref, dtype))), f"finish {where}: cgs_step_ref"
    assert same_bits(bv.get(), flat, dtype), f"{where}: the basis changed"
    for b in (pb, pb2, redA, redB, hc1):
        b.get()  # (guards)


@pytest.mark.parametrize("group", ["small", "tile", "ragged"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cgs_passes_exact(ctx, dtype, group):
    """pass A, pass B, pass C and mgs_finish on exact integers against cgs_step_ref, bit for bit: the partial sums of every row,
    hout and its accumulation onto hacc, w after each update, cgs_reduce, and the ncin = 1 form of the update against the
    partial-sum form (identical w, hout and partials); nothing written outside; every placement and k1 of the module docstring"""
    for n in br.sizes(dtype)[group]:
        if n == 0:
            continue
        for k1 in K1S + ((33,) if group == "ragged" else ()):
            for placement in PLACEMENTS:
                check_cgs_exact(ctx, dtype, n, k1, placement, seed=n + k1)


@pytest.mark.parametrize("placement", [(0, 0, "padded"), (0, 0, "odd")])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cgs_passes_exact_further_tiles(ctx, dtype, placement):
    """more than MAX_PARTIALS tiles: a workgroup's second tile (its per-wave sums accumulate in LDS), a nonzero of the basis beyond
    tile 1024; k1 = 3"""
    (n,) = br.sizes(dtype)["further"]
    assert br.marked(n, dtype)["beyond"]
    check_cgs_exact(ctx, dtype, n, 3, placement, seed=5)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_empty_vectors_and_k1_above_the_cap(ctx, dtype):
    """n = 0 returns 0 and writes nothing; k1 above the cap of 512 (and k1 < 1, an unknown update / dots combination, ldv < n)
    returns an error status and launches nothing"""
    T = br.NP[dtype]
    n = 64
    w0 = np.arange(n, dtype=T)
    bw, bv = Buf(ctx, dtype, n, 0, w0), Buf(ctx, dtype, 2 * n, 0, np.ones(2 * n, dtype=T))
    po, ho, ci = Buf(ctx, dtype, 3 * ROW, data=np.full(3 * ROW, SENT)), Buf(ctx, dtype, 4, data=np.full(4, SENT)), Buf(ctx, dtype, 4, data=np.ones(4))
    for update, dots in ((0, 1), (1, 1), (1, 2)):
        assert cgs_pass(ctx, dtype, 0, bw.p, bv.p, n, 2, update, dots, ci.p, 1, 1, None, ho.p, po.p, raw=True) == 0
    assert ctx.raw(f"cgs_reduce_{dtype}", 0, 2, po.p, ho.p) == 0
    bad = [dict(k1=cr.KMAX + 1), dict(k1=0), dict(k1=-3), dict(update=0, dots=2), dict(update=1, dots=0), dict(dots=3), dict(ldv=n - 1), dict(n=-1),
           dict(update=1, ncin=0), dict(update=1, ncin=br.MAX_PARTIALS + 1)]
    for kw in bad:
        a = dict(n=n, ldv=n, k1=2, update=1, dots=1, ncin=1)
        a.update(kw)
        rc = cgs_pass(ctx, dtype, a["n"], bw.p, bv.p, a["ldv"], a["k1"], a["update"], a["dots"], ci.p, a["ncin"], 1, None, ho.p, po.p, raw=True)
        assert rc != 0, kw
    assert ctx.raw(f"cgs_reduce_{dtype}", n, cr.KMAX + 1, po.p, ho.p) != 0
    ctx.torch.cuda.synchronize()
    assert same_bits(bw.get(), w0, dtype) and np.all(po.get() == T(SENT)) and np.all(ho.get() == T(SENT))
    assert ctx.lib.cuddh_hip_cgs_ws_bytes(cr.KMAX) == (cr.KMAX + 1) * ROW * 8
    # the largest k1 itself launches: 512 copies of one +-1 vector against w = that vector
    v = br.sparse_signs(n, dtype)
    k1 = cr.KMAX
    bv = Buf(ctx, dtype, k1 * n, 0, np.tile(v, k1))
    bw.set(v)
    po = Buf(ctx, dtype, (k1 + 1) * ROW, data=np.full((k1 + 1) * ROW, SENT))
    red = Buf(ctx, dtype, k1 + 1)
    assert cgs_pass(ctx, dtype, n, bw.p, bv.p, n, k1, 0, 1, None, 0, 0, None, None, po.p) == 0
    ctx.call(f"cgs_reduce_{dtype}", n, k1, po.p, red.p)
    assert np.all(red.get() == T(np.dot(v, v)))


# ================================================================== orthogonality on the device
class Arnoldi:
    """20 Arnoldi steps on the 300-dof diagonal operator of cr.separation_case, the basis in one device array (ldv = n)"""

    def __init__(self, ctx, dtype):
        self.ctx, self.dtype, self.T = ctx, dtype, br.NP[dtype]
        diag, b, self.steps = cr.separation_case()
        self.n = len(diag)
        self.diag = diag.astype(self.T)
        v0 = b.astype(self.T)
        v0 = v0 / self.T(np.sqrt(np.dot(v0, v0)))
        self.V = Buf(ctx, dtype, (self.steps + 1) * self.n, data=np.concatenate([v0, np.zeros(self.steps * self.n, dtype=self.T)]))
        self.dg = Buf(ctx, "f64", self.n, data=diag)

    def vec(self, k):
        return self.V.at(k * self.n)

    def apply(self, k):
        """v_{k+1} <- A v_k: diag_scale_f64 on the device in f64, on the host in f32"""
        if self.dtype == "f64":
            self.ctx.call("diag_scale_f64", self.n, 0, 1.0, self.dg.p, self.vec(k), self.vec(k + 1))
        else:
            host = self.V.get()
            host[(k + 1) * self.n:(k + 2) * self.n] = self.diag * host[k * self.n:(k + 1) * self.n]
            self.V.set(host)

    def basis(self):
        return self.V.get().reshape(self.steps + 1, self.n)


def norm_propagation_bound(w0, Vk, c1, c2, dtype):
    """||device w - reference w||_2 after the two projections, from the formats and the schedule alone (for the norm h[k1], which
    is small against |w0|): each coefficient is a reduction (br.reduction_bound on the sum of |terms| of its own inputs), each update
    k1 fused multiply-adds per element (gamma_k1 of the sum of the magnitudes), and every error of the first pass travels through
    the second"""
    n, k1 = len(w0), len(Vk)
    aV = np.abs(np.asarray(Vk, dtype=np.float64))
    aw = np.abs(w0.astype(np.float64))
    rb1 = np.array([br.reduction_bound(n, dtype, br.abs_dot(w0, v)) for v in Vk])
    size1 = aw + np.abs(c1.astype(np.float64)) @ aV
    dw1 = br.gamma(k1 + 1, dtype) * size1 + rb1 @ aV  # elementwise
    rb2 = np.array([br.reduction_bound(n, dtype, float(size1 @ a)) for a in aV]) + aV @ dw1
    size2 = size1 + np.abs(c2.astype(np.float64)) @ aV
    dw2 = dw1 + br.gamma(k1 + 1, dtype) * size2 + rb2 @ aV
    return float(np.linalg.norm(dw2))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cgs2_basis_is_orthogonal_on_the_device(ctx, dtype):
    """The separation of tests/test_cgs2_reference.py::test_orthogonality_separation, driven through the kernels: after 20 steps
    max|V^T V - I| <= 8 eps (the numpy reference gives <= 2 eps; the factor 4 covers the device's summation order), and every
    coefficient h_j of every Hessenberg column is within br.reduction_bound(n, dtype, sum |w_i v_j,i|) of cgs_step_ref applied in
    the wide type to the device's own w and basis (a working-precision CGS2 in numpy is at 0.03 of that bound; the largest ratio
    on the device is printed).  The norm h[k1] is small against |w|: it is held to br.norm_bound plus norm_propagation_bound."""
    A = Arnoldi(ctx, dtype)
    T, n, W = A.T, A.n, br.wide(dtype)
    rows = (A.steps + 1) * ROW
    pa, pb = Buf(ctx, dtype, rows, data=np.zeros(rows)), Buf(ctx, dtype, rows, data=np.zeros(rows))
    c1b, hb, c2b = (Buf(ctx, dtype, A.steps + 2, data=np.zeros(A.steps + 2)) for _ in range(3))
    worst = 0.0
    for k in range(A.steps):
        k1 = k + 1
        A.apply(k)
        before = A.basis()
        w0, Vk = before[k1].copy(), before[:k1]
        g, w = br.mgs_grid(n), A.vec(k1)
        cgs_pass(ctx, dtype, n, w, A.V.p, n, k1, 0, 1, None, 0, 0, None, None, pa.p)
        cgs_pass(ctx, dtype, n, w, A.V.p, n, k1, 1, 1, pa.at(ROW), g, ROW, None, c1b.p, pb.p)
        ctx.call(f"cgs_reduce_{dtype}", n, k1, pb.p, c2b.p)
        cgs_pass(ctx, dtype, n, w, A.V.p, n, k1, 1, 2, pb.at(ROW), g, ROW, c1b.p, hb.p, pa.p)
        ctx.call(f"mgs_finish_{dtype}", n, w, pa.p, hb.at(k1))
        h, c1, c2 = hb.get()[:k1 + 1], c1b.get()[:k1], c2b.get()[:k1]
        h_ref, _, _ = cr.cgs_step_ref(w0, Vk, dtype=dtype)
        bound = np.array([br.reduction_bound(n, dtype, br.abs_dot(w0, v)) for v in Vk])
        err = np.abs(h[:k1].astype(W) - h_ref[:k1]).astype(np.float64)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), f"{dtype} step {k}: h off by {np.max(err / bound):.2f} of br.reduction_bound at {int(np.argmax(err / bound))}"
        dnorm = norm_propagation_bound(w0, Vk, c1, c2, dtype)
        assert abs(W(h[k1]) - h_ref[k1]) <= dnorm + br.norm_bound(n, dtype, float(h_ref[k1])), f"{dtype} step {k}: norm {h[k1]!r} vs {h_ref[k1]!r}"
        assert np.array_equal(A.basis()[:k1].view(np.uint8), Vk.view(np.uint8)), "the basis changed"
    eps = float(np.finfo(T).eps)
    loss = cr.orthogonality_loss(list(A.basis()), dtype)
    print(f"{dtype}: device cgs2 max|V^T V - I| = {loss / eps:.2f} eps; largest |h_j - reference| / br.reduction_bound = {worst:.3f}")
    assert loss <= 8 * eps


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_mgs_chain_loses_orthogonality_on_the_same_input(ctx, dtype):
    """the chain krylov.cpp queues by default, on the same operator and start vector: more than 20 eps (numpy: 41 eps)"""
    A = Arnoldi(ctx, dtype)
    n, M = A.n, br.MAX_PARTIALS
    ws = Buf(ctx, dtype, 2 * M, data=np.zeros(2 * M))
    hb = Buf(ctx, dtype, A.steps + 2, data=np.zeros(A.steps + 2))
    for k in range(A.steps):
        A.apply(k)
        w, pa, pb = A.vec(k + 1), ws.at(0), ws.at(M)
        ctx.call(f"mgs_stage_{dtype}", n, w, None, A.vec(0), pa, pa, hb.p)
        for j in range(k + 1):
            ctx.call(f"mgs_stage_{dtype}", n, w, A.vec(j), A.vec(j + 1) if j < k else None, pa, pb, hb.at(j))
            pa, pb = pb, pa
        ctx.call(f"mgs_finish_{dtype}", n, w, pa, hb.at(k + 1))
    eps = float(np.finfo(A.T).eps)
    loss = cr.orthogonality_loss(list(A.basis()), dtype)
    print(f"{dtype}: device mgs max|V^T V - I| = {loss / eps:.2f} eps")
    assert loss > 20 * eps
