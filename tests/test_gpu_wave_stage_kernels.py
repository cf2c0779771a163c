"""kernels/waveholtz.hip, entry point by entry point through the C ABI, bit for bit against numpy.

Every vector holds small integers and every coefficient is a power of two (invm too), so each stage's result is exact in
float64 whatever the order and the contraction of its operations: the kernels are held to the numpy expressions of
include/cuddh_hip.h bit for bit.

Sizes (a tile is 512 sixteen-byte vectors = 1024 doubles): 1, 9, one tile - 1, one tile, one tile + 1, two tiles + 3.
Placements: every pointer on a 16-byte boundary (the 16-byte path, and its scalar tail where n is odd); every pointer one element
behind one; only the first input one element behind one (both: the element-wise path).  Both the forced form (F, G given) and the
homogeneous form (both NULL).  Every buffer has 16 elements of a NaN pattern on both sides; after each call the guards, and every
vector the stage does not write, are compared bitwise with what they held.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

GUARD = 16
PATTERN = 0x7FF8DEADBEEF0BAD
TILE = 1024
SIZES = (1, 9, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)
PLACEMENTS = ("aligned", "all_off_by_one", "first_off_by_one")

HALF_DT, DT, SIXTH_DT, CS, SN, FILT = 0.25, 0.5, 0.125, 2.0, -4.0, 0.5


class Buf:
    """n doubles at element offset `off` behind a 16-byte boundary, GUARD pattern elements on both sides"""

    def __init__(self, torch, dev, data, off):
        self.n, self.lo = len(data), GUARD + off
        host = np.full(self.lo + self.n + GUARD, PATTERN, dtype=np.uint64)
        host[self.lo:self.lo + self.n] = np.ascontiguousarray(data, dtype=np.float64).view(np.uint64)
        self.before = host.copy()
        self.t = torch.from_numpy(host.view(np.int64)).to(dev)
        assert self.t.data_ptr() % 16 == 0

    @property
    def p(self):
        return C.c_void_p(self.t.data_ptr() + 8 * self.lo)

    def bits(self):
        return self.t.cpu().numpy().view(np.uint64)

    def get(self):
        whole = self.bits()
        assert np.all(whole[:self.lo] == PATTERN), "elements before the vector were written"
        assert np.all(whole[self.lo + self.n:] == PATTERN), "elements behind the vector were written"
        return whole[self.lo:self.lo + self.n].view(np.float64).copy()

    def untouched(self):
        return np.array_equal(self.bits(), self.before)


def fq(x, w, q, forced):
    r = w - x["Hi"] * q
    if forced:
        r = r + CS * x["F"] + SN * x["G"]
    return x["invm"] * r


# name -> (leading scalars, pointer arguments in the entry point's order, the vectors it writes, numpy restatement)
def ref_begin(x, forced):
    return {"p": x["zu"], "q": x["zv"], "u": FILT * x["zu"], "v": FILT * x["zv"]}


def ref_rk2_a(x, forced):
    return {"qs": x["q"] + HALF_DT * fq(x, x["w"], x["q"], forced), "ps": x["p"] - HALF_DT * x["q"]}


def ref_rk2_b(x, forced):
    p = x["p"] - DT * x["qs"]
    q = x["q"] + DT * fq(x, x["w"], x["qs"], forced)
    return {"p": p, "q": q, "u": x["u"] + FILT * p, "v": x["v"] + FILT * q}


def ref_rk4_1(x, forced):
    k = fq(x, x["w"], x["q"], forced)
    return {"ps": x["p"] - HALF_DT * x["q"], "qs": x["q"] + HALF_DT * k, "aq": k, "ap": -x["q"]}


def ref_rk4_mid(h):
    def ref(x, forced):
        k = fq(x, x["w"], x["qs"], forced)
        return {"ps": x["p"] - h * x["qs"], "qs": x["q"] + h * k, "aq": x["aq"] + 2.0 * k, "ap": x["ap"] - 2.0 * x["qs"]}

    return ref


def ref_rk4_4(x, forced):
    k = fq(x, x["w"], x["qs"], forced)
    p = x["p"] + SIXTH_DT * (x["ap"] - x["qs"])
    q = x["q"] + SIXTH_DT * (x["aq"] + k)
    return {"p": p, "q": q, "u": x["u"] + FILT * p, "v": x["v"] + FILT * q}


STAGES = {
    "begin": ((FILT,), ("zu", "zv", "p", "q", "u", "v"), ref_begin),
    "rk2_a": ((HALF_DT, CS, SN), ("w", "p", "q", "invm", "Hi", "F", "G", "qs", "ps"), ref_rk2_a),
    "rk2_b": ((DT, CS, SN, FILT), ("w", "qs", "invm", "Hi", "F", "G", "p", "q", "u", "v"), ref_rk2_b),
    "rk4_1": ((HALF_DT, CS, SN), ("w", "p", "q", "invm", "Hi", "F", "G", "ps", "qs", "aq", "ap"), ref_rk4_1),
    "rk4_2": ((HALF_DT, CS, SN), ("w", "p", "q", "invm", "Hi", "F", "G", "ps", "qs", "aq", "ap"), ref_rk4_mid(HALF_DT)),
    "rk4_3": ((DT, CS, SN), ("w", "p", "q", "invm", "Hi", "F", "G", "ps", "qs", "aq", "ap"), ref_rk4_mid(DT)),
    "rk4_4": ((SIXTH_DT, CS, SN, FILT), ("w", "qs", "aq", "ap", "invm", "Hi", "F", "G", "p", "q", "u", "v"), ref_rk4_4),
}
VECTORS = ("zu", "zv", "w", "p", "q", "u", "v", "ps", "qs", "aq", "ap", "F", "G", "invm", "Hi")


def host_vectors(n, seed):
    rng = np.random.default_rng(seed)
    x = {name: rng.integers(-8, 9, n).astype(np.float64) for name in VECTORS}
    x["invm"] = 2.0 ** rng.integers(-1, 2, n)
    x["Hi"] = rng.integers(0, 3, n).astype(np.float64)
    return x


def test_every_stage_entry_point_is_covered():
    from cuddhelmholtz_amd import _native as N

    declared = {s for s in N.declared_symbols() if s.startswith("cuddh_hip_wave_stage_")}
    assert declared == {f"cuddh_hip_wave_stage_{name}_f64" for name in STAGES}


# (begin reads no load: it has one form)
@pytest.mark.parametrize("name,forced", [(name, forced) for name in STAGES for forced in (True, False) if forced or name != "begin"],
                         ids=lambda v: v if isinstance(v, str) else ("forced" if v else "homogeneous"))
def test_stage_matches_numpy_bit_for_bit(cuda, name, forced):
    import torch

    from cuddhelmholtz_amd import _native as N

    scalars, pointers, ref = STAGES[name]
    fn = getattr(N.lib, f"cuddh_hip_wave_stage_{name}_f64")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n in SIZES:
        for placement in PLACEMENTS:
            x = host_vectors(n, seed=n)
            want = ref(x, forced)
            off = {v: 1 if placement == "all_off_by_one" or (placement == "first_off_by_one" and v == pointers[0]) else 0 for v in pointers}
            bufs = {v: Buf(torch, cuda, x[v], off[v]) for v in pointers}
            args = [None if (v in ("F", "G") and not forced) else bufs[v].p for v in pointers]
            N.check(fn(n, *scalars, *args, st), name)
            torch.cuda.synchronize()
            for v in pointers:
                where = f"{name} n={n} {placement} {v}"
                if v in want:
                    got = bufs[v].get()
                    assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(want[v]).view(np.uint64)), where
                else:
                    assert bufs[v].untouched(), where
