"""BLAS-1, fused Gram-Schmidt and exchange kernels restated in numpy (TEST INFRASTRUCTURE, not collected).

Three things live here, shared by tests/test_blas1_reference.py (CPU: pins this module) and tests/test_gpu_blas1_kernels.py
(GPU: holds kernels/blas1.hip to it):

  * the kernel's constants and the vector sizes derived from them (`sizes`): every size at which blas1.hip takes another path;
  * case generators.  The EXACT ones draw small integers such that the sum of |term| of a reduction stays below 2^24 (f32) or
    2^53 (f64): every partial sum is then an integer the format holds exactly, whatever the order of summation, and the device
    result must equal the integer reference bit for bit.  The last full 16-byte vector, the scalar tail behind it and the first
    element of the second tile carry values that differ from their neighbours, so that a vector counted twice (the kernels load
    with a clamped index and guard only the use), a dropped tail or a shifted element changes the integer;
  * restatements in high precision (float64 for f32 data, longdouble for f64) and a-priori error bounds.
"""
from __future__ import annotations

import math

import numpy as np

# ---- constants of kernels/blas1.hip and kernels/common.hpp (stream_grid)
WAVE = 64
BLOCK = 256  # threads of a workgroup
UNROLL = 4  # 16-byte accesses of a thread per tile
TILE = UNROLL * BLOCK  # 16-byte vectors per tile: 1024
MAX_PARTIALS = 1024  # workgroups of a reduction = slots of one half of the workspace
NT_BYTES = 64 << 20  # from this size on the maps and reductions use the non-temporal instantiations
STREAM_GRID_CAP = 256 * 8  # workgroups of the indexed (grid-stride) kernels
PACK = {"f64": 2, "f32": 4, "i32": 4}  # elements of a 16-byte vector
NP = {"f64": np.float64, "f32": np.float32, "i32": np.int32}
EXACT_LIMIT = {"f64": 2 ** 53, "f32": 2 ** 24}  # integers up to here are exact

INDEXED_SIZES = (0, 1, 255, 256, 257, STREAM_GRID_CAP * BLOCK + 257)  # the last one: second trip of the grid-stride loop


def sizes(dtype: str) -> dict:
    """size group -> vector lengths (the table of the test's docstring)"""
    n = PACK[dtype]
    item = np.dtype(NP[dtype]).itemsize
    return {
        "small": sorted({0, 1, n - 1, n, n + 1, BLOCK * n - 1}),
        "tile": [TILE * n - 1, TILE * n, TILE * n + 1],
        "ragged": [3 * TILE * n + 5 * n + (n - 1)],
        "further": [n * (TILE * (MAX_PARTIALS + 1) + 300) + (n - 1)],  # more than MAX_PARTIALS tiles: the second trip of the tile loops
        "nt": [NT_BYTES // item - 1, NT_BYTES // item],
    }


def tile_grid(n_vectors: int, cap: int) -> int:
    return max(1, min(-(-n_vectors // TILE), cap))


def reduce_grid(n: int, dtype: str) -> int:
    return tile_grid(n // PACK[dtype], MAX_PARTIALS)


def mgs_grid(n: int) -> int:
    return tile_grid(n // 2, MAX_PARTIALS)  # (both precisions: blas1.hip::mgs_grid)


def stream_grid(n: int) -> int:
    return max(1, min(-(-n // BLOCK), STREAM_GRID_CAP))


MAP_OFFSETS = {"f64": [(0, 0), (1, 1), (0, 1), (1, 0)], "f32": [(0, 0), (1, 1), (0, 1), (1, 0), (2, 0), (0, 2)]}
MAP_OFFSETS["i32"] = MAP_OFFSETS["f32"]
MGS_OFFSETS = [(0, 0, 0), (1, 1, 1), (0, 1, 0), (0, 0, 1), (1, 0, 0)]  # (w, vprev, vnext)


# ---------------------------------------------------------------- marked positions
def marked(n: int, dtype: str) -> dict:
    """name -> element indices (possibly empty): the places where a clamped load, a tail loop or a tile loop goes wrong"""
    N = PACK[dtype]
    nv = n // N
    out = {
        "first": [0] if n > 0 else [],
        "tile_end": [i for i in (TILE * N - 1,) if i < n],  # last element of the first tile
        "tile2": [i for i in (TILE * N,) if i < n],  # first element of the second tile
        "beyond": [i for i in (N * TILE * MAX_PARTIALS + 3,) if i < n],  # in tile MAX_PARTIALS: a workgroup's second tile
        "last_vector": list(range((nv - 1) * N, nv * N)) if nv > 0 else [],
        "tail": list(range(nv * N, n)),
    }
    return out


# ---------------------------------------------------------------- exact-integer generators
def exact_dot(n: int, dtype: str, rng, xmax: int = 3):
    """x in {1..xmax} (xmax == 1: {0, 1}), y in {-1, +1}.  Every term of the last full vector is +xmax (the vector before it: -1),
    every term of the tail is -max(1, xmax - 1), the first element of the second tile +xmax between two -1."""
    x = rng.integers(1, xmax + 1, n, dtype=np.int8) if xmax > 1 else rng.integers(0, 2, n, dtype=np.int8)
    y = 2 * rng.integers(0, 2, n, dtype=np.int8) - 1
    m = marked(n, dtype)
    for i in m["tile2"]:
        x[i], y[i] = xmax, 1
        for j in (i - 1, i + 1):
            if 0 <= j < n:
                x[j], y[j] = 1, -1
    lv = m["last_vector"]
    if lv:
        x[lv], y[lv] = xmax, 1  # counted twice: + N xmax
        if lv[0] >= PACK[dtype]:
            prev = [i - PACK[dtype] for i in lv]
            x[prev], y[prev] = 1, -1
    if m["tail"]:
        x[m["tail"]], y[m["tail"]] = max(1, xmax - 1), -1  # dropped: + len(tail) (xmax - 1)
    return x.astype(NP[dtype]), y.astype(NP[dtype])


def exact_sqdist(n: int, dtype: str, rng):
    """x, y in {0, 1}; the marked vector and the tail have (x - y)^2 == 1, the vector before the marked one 0"""
    x, y = rng.integers(0, 2, n, dtype=np.int8), rng.integers(0, 2, n, dtype=np.int8)
    m = marked(n, dtype)
    for i in m["tile2"]:
        x[i], y[i] = 1, 0
        if i - 1 >= 0:
            x[i - 1] = y[i - 1] = 1
    lv = m["last_vector"]
    if lv:
        x[lv], y[lv] = 1, 0
        if lv[0] >= PACK[dtype]:
            prev = [i - PACK[dtype] for i in lv]
            x[prev] = y[prev] = 1
    if m["tail"]:
        x[m["tail"]], y[m["tail"]] = 0, 1
    return x.astype(NP[dtype]), y.astype(NP[dtype])


def exact_nrm2(n: int, dtype: str, rng):
    """x in {-1, 0, 1} with k^2 nonzeros, k = isqrt(n): the norm is the integer k.  The n - k^2 <= 2 k zeros are the vector before
    the last full one, then random places; the tail, the last full vector and the first element of the second tile stay nonzero
    (for tiny n, as far as k^2 reaches)."""
    N = PACK[dtype]
    k = math.isqrt(n)
    z = n - k * k
    m = marked(n, dtype)
    keep = list(dict.fromkeys(m["tail"] + m["last_vector"] + m["tile2"] + m["beyond"]))
    zeros = [i - N for i in m["last_vector"] if i - N >= 0 and i - N not in keep][:z]
    excluded = set(keep) | set(zeros)
    while len(zeros) < z:
        if len(excluded) >= n:  # tiny n: marked places give way, the tail last
            zeros += [i for i in reversed(keep) if i not in zeros][: z - len(zeros)]
            break
        for c in rng.permutation(np.unique(rng.integers(0, n, 2 * (z - len(zeros)) + 16))):
            if int(c) not in excluded and len(zeros) < z:
                zeros.append(int(c))
                excluded.add(int(c))
    x = 2 * rng.integers(0, 2, n, dtype=np.int8) - 1
    x[zeros] = 0
    return x.astype(NP[dtype]), k


def sparse_signs(n: int, dtype: str, shift: int = 0):
    """A handful of +-1 at the marked places (moved by `shift` elements where that stays inside the vector), 0 elsewhere"""
    v = np.zeros(n, dtype=NP[dtype])
    m = marked(n, dtype)
    places = m["first"] + m["tile_end"] + m["tile2"] + m["beyond"] + m["last_vector"][:1] + m["tail"][-1:]
    s = 1
    for p in places:
        q = p + shift if 0 <= p + shift < n else p
        v[q] = s
        s = -s
    return v


def exact_mgs(n: int, dtype: str, rng):
    """w in {-2..2} ({-1..1} where 4 n would pass the exactness limit), two sparse +-1 vectors, a dense +-1 vector"""
    wmax = 2 if 4 * n + 4096 <= EXACT_LIMIT[dtype] else 1
    w = rng.integers(-wmax, wmax + 1, n, dtype=np.int8)
    p1, p2 = sparse_signs(n, dtype), sparse_signs(n, dtype, shift=1)
    for p in (p2, p1):
        w[p != 0] = wmax * p[p != 0].astype(np.int8)  # every term of <w, p1> is + wmax: the coefficient is not zero
    dense = 2 * rng.integers(0, 2, n, dtype=np.int8) - 1
    return w.astype(NP[dtype]), p1, p2, dense.astype(NP[dtype])


def abs_terms(x, y=None) -> int:
    """sum of |term| of <x, y> (y None: <x, x>) as a Python integer: the quantity the exactness limit is about"""
    xi = np.asarray(x).astype(np.int64)
    yi = xi if y is None else np.asarray(y).astype(np.int64)
    return int(np.sum(np.abs(xi * yi)))


def int_dot(x, y) -> int:
    return int(np.dot(np.asarray(x).astype(np.int64), np.asarray(y).astype(np.int64)))


def int_sqdist(x, y) -> int:
    d = np.asarray(x).astype(np.int64) - np.asarray(y).astype(np.int64)
    return int(np.dot(d, d))


# ---------------------------------------------------------------- high-precision restatements
def wide(dtype: str):
    return np.longdouble if dtype == "f64" else np.float64


def dot_wide(x, y, dtype: str):
    """<x, y> in the wide type, pairwise (numpy's add.reduce): error ~ log2(n) ulps of the WIDE type of sum |terms|"""
    W = wide(dtype)
    return np.sum(np.asarray(x).astype(W) * np.asarray(y).astype(W))


def abs_dot(x, y) -> float:
    return float(np.sum(np.abs(np.asarray(x, dtype=np.float64) * np.asarray(y, dtype=np.float64))))


def axpby_wide(a, x, b, y, dtype: str):
    W = wide(dtype)
    return W(a) * np.asarray(x).astype(W) + W(b) * np.asarray(y).astype(W)


def mgs_stage_ref(w, vprev, vnext, pin_sum):
    """one fused stage in the precision of `w`: (h, new w, sum of the partials it leaves)"""
    h = pin_sum
    if vprev is not None:
        w = w - h * vprev
    return h, w, np.dot(w, w if vnext is None else vnext)


def mgs_finish_ref(w, pin_sum):
    nrm = np.sqrt(pin_sum)
    return nrm, w / nrm


def mgs_chain_ref(w, V):
    """What krylov.cpp::queue_step queues for k = len(V) - 1: first stage, one projection stage per basis vector, finish.
    Returns (h[0..k+1], normalised w) in the precision of the inputs."""
    k1 = len(V)
    h = []
    _, w, s = mgs_stage_ref(w, None, V[0], None)
    for j in range(k1):
        hj, w, s = mgs_stage_ref(w, V[j], V[j + 1] if j + 1 < k1 else None, s)
        h.append(hj)
    nrm, w = mgs_finish_ref(w, s)
    h.append(nrm)
    return np.asarray(h), w


def mgs_classical(w, V):
    """textbook modified Gram-Schmidt: h = <w, v>; w -= h v; then normalise"""
    h = []
    for v in V:
        hj = np.dot(w, v)
        w = w - hj * v
        h.append(hj)
    nrm = np.sqrt(np.dot(w, w))
    h.append(nrm)
    return np.asarray(h), w / nrm


def orthonormal_columns(n: int, k: int, rng, dtype: str):
    """k orthonormal vectors of length n (QR in float64), rounded to `dtype`"""
    q, _ = np.linalg.qr(rng.standard_normal((n, k)))
    return [np.ascontiguousarray(q[:, j]).astype(NP[dtype]) for j in range(k)]


def csr_sum_ref(off, src, x, y0, accumulate: bool):
    """strictly left-to-right float64 row sums, vectorised over the rows (one pass per position in the row)"""
    off = np.asarray(off, dtype=np.int64)
    n_rows = len(off) - 1
    ln = off[1:] - off[:-1]
    s = np.array(y0[:n_rows], dtype=np.float64) if accumulate else np.zeros(n_rows)
    for k in range(int(ln.max()) if n_rows else 0):
        rows = np.flatnonzero(ln > k)
        s[rows] = s[rows] + x[src[off[rows] + k]]
    return s


def csr_case(n_rows: int, n_x: int, rng):
    """rows of length 0, 1, 2, 7 and 64, mixed; x holds 1e16, 1 and -1e16 among random entries, and the first long rows list
    them such that the order of the additions decides the result"""
    lens = rng.choice(np.array([0, 1, 2, 7, 64]), size=n_rows, p=[0.2, 0.25, 0.25, 0.27, 0.03]) if n_rows else np.zeros(0, dtype=np.int64)
    for i, v in enumerate((64, 0, 7, 1, 2)):
        if i < n_rows:
            lens[i] = v
    off = np.zeros(n_rows + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    x = rng.standard_normal(n_x)
    x[:3] = (1e16, 1.0, -1e16)
    src = rng.integers(0, n_x, int(off[-1]))
    for r in np.flatnonzero(lens >= 7)[:64]:
        src[off[r]:off[r] + 3] = rng.permutation(3)  # (1e16 + 1) - 1e16 = 0 but (1e16 - 1e16) + 1 = 1
    return off.astype(np.int32), src.astype(np.int32), x


# ---------------------------------------------------------------- a-priori bounds
def unit_roundoff(dtype: str) -> float:
    return float(np.finfo(NP[dtype]).eps) / 2


def reduction_depth(n: int, dtype: str) -> int:
    """An upper bound, monotone in n, of the number of additions a term of a reduction of blas1.hip passes through:
    the terms one thread accumulates, 6 shuffle steps, 4 waves, then the second stage (<= 4 partials per thread, 6 shuffle steps,
    4 waves).  Per thread: UNROLL * N terms per tile and one tail element on the vector path, ceil(n_tiles / MAX_PARTIALS) tiles;
    on the scalar path ceil(n / (grid * BLOCK)) <= 2 * UNROLL * N + 1 while the grid is below its cap and n / (MAX_PARTIALS * BLOCK)
    rounded up beyond."""
    N = PACK[dtype]
    n_tiles = -(-(n // N) // TILE)
    per_thread = max(UNROLL * N * max(1, -(-n_tiles // MAX_PARTIALS)) + 1, 2 * UNROLL * N + 1, -(-n // (MAX_PARTIALS * BLOCK)))
    return per_thread + 6 + 4 + 4 + 6 + 4


def gamma(d: int, dtype: str) -> float:
    """Higham's gamma_d = d u / (1 - d u)"""
    u = unit_roundoff(dtype)
    return d * u / (1 - d * u)


def reduction_bound(n: int, dtype: str, sum_abs_terms: float) -> float:
    """|device sum - exact sum| <= gamma_{d+1} * sum |terms| (one more rounding for a product that is not fused)"""
    return gamma(reduction_depth(n, dtype) + 1, dtype) * sum_abs_terms


def axpby_bound(a, x, b, y, dtype: str):
    """elementwise: 4 eps (|a x| + |b y|)"""
    eps = float(np.finfo(NP[dtype]).eps)
    return 4 * eps * (abs(float(a)) * np.abs(np.asarray(x, dtype=np.float64)) + abs(float(b)) * np.abs(np.asarray(y, dtype=np.float64)))


def quotient_bound(result, dtype: str):
    """elementwise, for the divisions: 4 eps |result|"""
    return 4 * float(np.finfo(NP[dtype]).eps) * np.abs(np.asarray(result, dtype=np.float64))


def projection_bound(w, h, v, dtype: str):
    """elementwise, w - h v evaluated as one fused multiply-add or as a product and a sum: 2 eps (|w| + |h v|)"""
    eps = float(np.finfo(NP[dtype]).eps)
    return 2 * eps * (np.abs(np.asarray(w, dtype=np.float64)) + abs(float(h)) * np.abs(np.asarray(v, dtype=np.float64)))


# Loss of orthogonality max_j |<w, v_j>| of the normalised result of the chain, in units of eps, for a standard normal w against three
# orthonormal vectors.  Measured on the reference chain (mgs_chain_ref) run on the CPU in the kernel's own precision, evaluated in
# the wide type (tests/test_blas1_reference.py::test_orthogonality_constant measures it again): 0.146 eps in f64 and 0.041 eps in
# f32 at most over the sizes and seeds of the GPU test.  The bound is 1 eps: the larger figure with a margin of more than 4.
ORTHOGONALITY_EPS = 1.0


def orthogonality_bound(dtype: str) -> float:
    return ORTHOGONALITY_EPS * float(np.finfo(NP[dtype]).eps)


def norm_bound(n: int, dtype: str, norm: float) -> float:
    """|device norm - sqrt(<w, w>)|: the sum of squares to gamma_d, the square root to one rounding"""
    return norm * (gamma(reduction_depth(n, dtype), dtype) + unit_roundoff(dtype))


def unit_norm_bound(n: int, dtype: str) -> float:
    """| |w / nrm|^2 - 1 | with nrm^2 off by gamma_d, one rounding in the square root and one in every division"""
    u, g = unit_roundoff(dtype), gamma(reduction_depth(n, dtype), dtype)
    return (1 + u) ** 2 / ((1 - g) * (1 - u) ** 2) - 1
