"""Pins tests/blas1_reference.py, the helper tests/test_gpu_blas1_kernels.py holds the BLAS-1 kernels to (CPU only):
the exact-integer generators stay exact at every size of the table, the restated fused Gram-Schmidt chain is classical modified
Gram-Schmidt, the bounds grow with n, and the constant of the orthogonality check is what the reference chain gives."""
import math

import numpy as np
import pytest

import blas1_reference as br

GROUPS = ("small", "tile", "ragged", "further", "nt")


def all_sizes(dtype, groups=GROUPS):
    return [n for g in groups for n in br.sizes(dtype)[g]]


def test_sizes_follow_from_the_kernel_constants():
    assert (br.TILE, br.MAX_PARTIALS, br.PACK["f64"], br.PACK["f32"], br.PACK["i32"]) == (1024, 1024, 2, 4, 4)
    s64, s32 = br.sizes("f64"), br.sizes("f32")
    assert s64["small"] == [0, 1, 2, 3, 511] and s32["small"] == [0, 1, 3, 4, 5, 1023]
    assert s64["tile"] == [2047, 2048, 2049] and s32["tile"] == [4095, 4096, 4097]
    assert s64["ragged"] == [6155] and s32["ragged"] == [12311]
    for dtype, s in (("f64", s64), ("f32", s32)):
        N, item = br.PACK[dtype], np.dtype(br.NP[dtype]).itemsize
        (n,) = s["further"]
        assert -(-(n // N) // br.TILE) > br.MAX_PARTIALS and n % N == N - 1  # a second trip of the tile loops, ragged end
        assert br.reduce_grid(n, dtype) == br.MAX_PARTIALS == br.mgs_grid(n)
        assert br.marked(n, dtype)["beyond"] and len(br.marked(n, dtype)["tail"]) == N - 1
        lo, hi = s["nt"]
        assert lo * item < br.NT_BYTES <= hi * item and hi == lo + 1
    assert br.stream_grid(br.INDEXED_SIZES[-1]) == br.STREAM_GRID_CAP and br.INDEXED_SIZES[-1] > br.STREAM_GRID_CAP * br.BLOCK


def integers_in(x, lo, hi):
    return x.size == 0 or bool(lo <= x.min() and x.max() <= hi and np.all(x == np.rint(x)))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_exact_generators_stay_exact(dtype):
    limit = br.EXACT_LIMIT[dtype]
    for n in all_sizes(dtype):
        rng = np.random.default_rng(n)
        m = br.marked(n, dtype)
        lv, tail = m["last_vector"], m["tail"]
        xmax = 3 if 3 * n <= limit else 1
        x, y = br.exact_dot(n, dtype, rng, xmax)
        assert n * xmax <= limit and br.abs_terms(x, y) <= n * xmax
        assert integers_in(x, 1 if xmax > 1 else 0, xmax) and integers_in(y, -1, 1) and np.all(y != 0)
        # the marked places differ from their neighbours: the term of a doubled last vector or of a dropped tail is not zero
        assert br.int_dot(x[lv], y[lv]) == xmax * len(lv) and br.int_dot(x[tail], y[tail]) == -max(1, xmax - 1) * len(tail)
        x, y = br.exact_sqdist(n, dtype, rng)
        assert n <= limit and integers_in(x, 0, 1) and integers_in(y, 0, 1)
        assert br.int_sqdist(x[lv], y[lv]) == len(lv) and br.int_sqdist(x[tail], y[tail]) == len(tail)
        x, k = br.exact_nrm2(n, dtype, rng)
        assert integers_in(x, -1, 1) and br.abs_terms(x) == k * k <= n <= limit and k == math.isqrt(n)
        if k * k >= len(lv) + len(tail):
            assert np.all(x[lv + tail] != 0)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_exact_mgs_inputs_stay_exact(dtype):
    """Every inner product of the single-stage test (w, then w - h1 p1, then that - h2 p2, against the sparse vectors, the dense one
    and itself) has sum |terms| within the exactness limit, and the coefficients are small integers."""
    limit = br.EXACT_LIMIT[dtype]
    for n in all_sizes(dtype, ("small", "tile", "ragged", "further")):
        w, p1, p2, dense = br.exact_mgs(n, dtype, np.random.default_rng(n))
        assert 0 < np.count_nonzero(p1) <= 8 or n == 0
        assert set(np.unique(dense)) <= {-1.0, 1.0} and np.abs(w).max(initial=0) <= 2
        h1 = br.int_dot(w, p1)
        w1 = w - br.NP[dtype](h1) * p1
        h2 = br.int_dot(w1, p2)
        w2 = w1 - br.NP[dtype](h2) * p2
        assert abs(h1) <= 16 and abs(h2) <= 16 * 17
        for a, b in ((w, p1), (w1, dense), (w1, p2), (w2, None)):
            assert br.abs_terms(a, b) <= limit
        assert np.array_equal(w2, w2.astype(np.int64))  # still integers in the format
        if n > 1:
            assert h1 > 0


def test_restated_chain_is_classical_gram_schmidt():
    rng = np.random.default_rng(7)
    for n in (2, 5, 64, 777):
        for k in (1, 2, 3):
            if k >= n:
                continue
            V = [v.astype(np.longdouble) for v in br.orthonormal_columns(n, k, rng, "f64")]
            w = rng.standard_normal(n).astype(np.longdouble)
            h, q = br.mgs_chain_ref(w, V)
            hc, qc = br.mgs_classical(w, V)
            assert h.dtype == np.longdouble and len(h) == k + 1
            # the same operations in the same order: equal to a few units of the longdouble roundoff, not merely close
            tol = 8 * float(np.finfo(np.longdouble).eps)
            assert np.all(np.abs(h - hc) <= tol * np.maximum(1, np.abs(hc)))
            assert np.all(np.abs(q - qc) <= tol)
            assert abs(float(np.dot(q, q)) - 1) <= 1e-15
            if n > k:
                assert max(abs(float(np.dot(q, v))) for v in V) <= 1e-15


def test_bounds_are_monotone_in_n():
    for dtype in ("f64", "f32"):
        ns = sorted(set(all_sizes(dtype)) | set(range(0, 70000, 997)) | {2 ** k + d for k in range(8, 25) for d in (-1, 0, 1)})
        depth = [br.reduction_depth(n, dtype) for n in ns]
        assert depth == sorted(depth) and depth[0] >= 2 * br.UNROLL * br.PACK[dtype] + 1 + 24
        for f in (lambda n: br.reduction_bound(n, dtype, 1.0), lambda n: br.norm_bound(n, dtype, 1.0), lambda n: br.unit_norm_bound(n, dtype)):
            v = [f(n) for n in ns]
            assert v == sorted(v) and v[0] > 0
        # the depth covers the schedule: terms of one thread on the vector path and on the scalar path
        for n in ns:
            N = br.PACK[dtype]
            for grid in (br.reduce_grid(n, dtype), br.mgs_grid(n)):
                tiles = -(-(n // N) // br.TILE)
                vector_path = br.UNROLL * N * -(-tiles // grid) + 1
                scalar_path = -(-n // (grid * br.BLOCK))
                assert br.reduction_depth(n, dtype) >= max(vector_path, scalar_path) + 24
    assert br.gamma(10, "f64") > 10 * br.unit_roundoff("f64")
    x = np.array([1.0, -2.0]), np.array([3.0, 0.5])
    assert np.array_equal(br.axpby_bound(2, x[0], -1, x[1], "f64"), 4 * np.finfo(np.float64).eps * np.array([5.0, 4.5]))


def test_csr_reference_adds_left_to_right():
    off, src, x = br.csr_case(300, 607, np.random.default_rng(3))
    lens = np.diff(off)
    assert set(np.unique(lens)) == {0, 1, 2, 7, 64} and list(lens[:5]) == [64, 0, 7, 1, 2]
    y0 = np.full(300, 5.5)
    for acc in (False, True):
        got = br.csr_sum_ref(off, src, x, y0, acc)
        for r in range(300):
            s = 5.5 if acc else 0.0
            for k in range(off[r], off[r + 1]):
                s = s + x[src[k]]
            assert got[r] == s
    # the order decides: some row's sum differs from the sorted-order sum
    got = br.csr_sum_ref(off, src, x, y0, False)
    other = np.array([math.fsum(x[src[off[r]:off[r + 1]]]) for r in range(300)])
    assert np.any(got != other)


def test_orthogonality_constant(capsys):
    """The reference chain in the kernel's own precision loses at most a quarter of orthogonality_bound()."""
    worst = {}
    for dtype in ("f64", "f32"):
        eps = float(np.finfo(br.NP[dtype]).eps)
        (n,) = br.sizes(dtype)["ragged"]
        worst[dtype] = 0.0
        for seed in range(3):
            rng = np.random.default_rng(seed)
            V = br.orthonormal_columns(n, 3, rng, dtype)
            w = rng.standard_normal(n).astype(br.NP[dtype])
            h, q = br.mgs_chain_ref(w, V)
            assert q.dtype == br.NP[dtype]
            worst[dtype] = max(worst[dtype], max(abs(float(br.dot_wide(q, v, dtype))) for v in V) / eps)
        assert 4 * worst[dtype] * eps <= br.orthogonality_bound(dtype)
    with capsys.disabled():
        print(f"\n[blas1 reference] loss of orthogonality of the reference chain: f64 {worst['f64']:.3f} eps, f32 {worst['f32']:.3f} eps")
