"""numpy restatement of the paired lattice sweeps (include/cuddh_hip.h, cuddh_hip_wave_pair_*), written from the pointwise table:

    pair      tile 1   tile 2 (derived, pointwise)      stages
    rk2       p        ph  = p - dt/2 q                 rk2_a, rk2_b
    rk4_12    p        ps1 = p - dt/2 q                 rk4_1, rk4_2
    rk4_34    ps2      ps3 = p - dt qs                  rk4_3 (h = dt), rk4_4

Each function forms the derived tile, takes the stiffness of both tiles and then evaluates the two stage formulas with the first
stage's results as plain local values.  K is a callable, lattice vector -> K vector.  Vectors are a dict of 1-D arrays of one
dtype; scalars are converted to that dtype, so that the same text runs in float32, float64 and longdouble.  On integer-valued
data with power-of-two scalars every operation is exact and fused or unfused arithmetic agree.
"""
import numpy as np

from test_gpu_wave_lattice_kernels import CX, CY, line


def stiffness(nx, ny, nb, stride, A, w, dtype=np.float64, reverse=False):
    """K as a callable on padded lattice vectors of `dtype`: per node the terms of test_gpu_wave_lattice_kernels.line, summed
    from zero in ascending (reverse: descending) order of the offset; zero in the padding columns"""
    H = nb - 1
    Lx, Ly = nx * H + 1, ny * H + 1
    lx, ly = line(nx, nb, A, w), line(ny, nb, A, w)
    T = dtype

    def K(p):
        P = np.asarray(p, dtype=T).reshape(Ly, stride)
        sx, sy = np.zeros((Ly, stride), dtype=T), np.zeros((Ly, stride), dtype=T)
        for I, (terms, _) in enumerate(lx):
            for d, c in (reversed(terms) if reverse else terms):
                sx[:, I] = sx[:, I] + T(c) * P[:, I + d]
        for J, (terms, _) in enumerate(ly):
            for d, c in (reversed(terms) if reverse else terms):
                sy[J, :Lx] = sy[J, :Lx] + T(c) * P[J + d, :Lx]
        Wx, Wy = np.zeros(stride, dtype=T), np.array([wt for _, wt in ly], dtype=T)
        Wx[:Lx] = [wt for _, wt in lx]
        out = (T(CX) * Wy)[:, None] * sx + (T(CY) * Wx)[None, :] * sy
        out[:, Lx:] = 0
        assert out.dtype == T
        return out.reshape(-1)

    return K


def _accel(x, w, q, c, s, forced):
    """invm (w - Hi q + c F + s G)"""
    T = w.dtype.type
    r = w - x["Hi"] * q
    if forced:
        r = r + T(c) * x["F"] + T(s) * x["G"]
    return x["invm"] * r


def pair_rk2(K, x, half_dt, dt, c0, s0, c1, s1, filt, forced):
    """reads p q u v invm Hi (F G); returns the new p q u v"""
    T = x["p"].dtype.type
    p, q = x["p"], x["q"]
    ph = p - T(half_dt) * q
    wa, wb = K(p), K(ph)
    qh = q + T(half_dt) * _accel(x, wa, q, c0, s0, forced)
    pn = p - T(dt) * qh
    qn = q + T(dt) * _accel(x, wb, qh, c1, s1, forced)
    return {"p": pn, "q": qn, "u": x["u"] + T(filt) * pn, "v": x["v"] + T(filt) * qn}


def pair_rk4_12(K, x, half_dt, c0, s0, c1, s1, forced):
    """reads p q invm Hi (F G); returns ps2 qs aq ap"""
    T = x["p"].dtype.type
    p, q = x["p"], x["q"]
    ps1 = p - T(half_dt) * q
    wa, wb = K(p), K(ps1)
    k1 = _accel(x, wa, q, c0, s0, forced)
    qs1 = q + T(half_dt) * k1
    k2 = _accel(x, wb, qs1, c1, s1, forced)
    return {"ps2": p - T(half_dt) * qs1, "qs": q + T(half_dt) * k2, "aq": k1 + T(2) * k2, "ap": -q - T(2) * qs1}


def pair_rk4_34(K, x, dt, sixth_dt, c1, s1, c2, s2, filt, forced):
    """reads ps2 p qs q aq ap u v invm Hi (F G); returns the new p q u v"""
    T = x["p"].dtype.type
    p, q, qs = x["p"], x["q"], x["qs"]
    ps3 = p - T(dt) * qs
    wa, wb = K(x["ps2"]), K(ps3)
    k3 = _accel(x, wa, qs, c1, s1, forced)
    qs3 = q + T(dt) * k3
    aq3 = x["aq"] + T(2) * k3
    ap3 = x["ap"] - T(2) * qs
    k4 = _accel(x, wb, qs3, c2, s2, forced)
    pn = p + T(sixth_dt) * (ap3 - qs3)
    qn = q + T(sixth_dt) * (aq3 + k4)
    return {"p": pn, "q": qn, "u": x["u"] + T(filt) * pn, "v": x["v"] + T(filt) * qn}


def march_pairs(K, x, nt, rk4, scalars, forced):
    """nt steps of the paired schedule with its buffer swaps (csrc/src/waveholtz.cpp); returns (u, v).  x is not changed.
    scalars: dict half_dt dt sixth_dt c s filt, the same c, s and filt in every sweep and step (the per-sweep restatements of
    test_gpu_wave_stage_kernels.py read theirs from module constants)"""
    k = scalars
    b = {name: v.copy() for name, v in x.items()}
    if not rk4:
        b["p2"], b["q2"] = np.full_like(b["p"], np.nan), np.full_like(b["q"], np.nan)
        P, Q, P2, Q2 = "p", "q", "p2", "q2"
        for _ in range(nt):
            y = pair_rk2(K, {**b, "p": b[P], "q": b[Q]}, k["half_dt"], k["dt"], k["c"], k["s"], k["c"], k["s"], k["filt"], forced)
            b[P2], b[Q2], b["u"], b["v"] = y["p"], y["q"], y["u"], y["v"]
            P, P2, Q, Q2 = P2, P, Q2, Q
    else:
        b["p2"] = np.full_like(b["p"], np.nan)
        P, P2 = "p", "p2"
        for _ in range(nt):
            y = pair_rk4_12(K, {**b, "p": b[P]}, k["half_dt"], k["c"], k["s"], k["c"], k["s"], forced)
            b["ps2"], b["qs"], b["aq"], b["ap"] = y["ps2"], y["qs"], y["aq"], y["ap"]
            y = pair_rk4_34(K, {**b, "p": b[P]}, k["dt"], k["sixth_dt"], k["c"], k["s"], k["c"], k["s"], k["filt"], forced)
            b[P2], b["q"], b["u"], b["v"] = y["p"], y["q"], y["u"], y["v"]
            P, P2 = P2, P
    return b["u"], b["v"]
