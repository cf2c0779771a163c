"""DDH with per-subdomain time grids, restated on the test side (TEST INFRASTRUCTURE).

Subdomain s marches ratios[s] * nt steps of dt / ratios[s] per period, nt and dt being the mesh grid's (DDH(time_step=...),
DESIGN 4.3).  Local solves couple through the traces only, so the oracle needs no new code for this: `PerSubdomainOracle` calls
the oracle's solve(d0=s, d1=s+1) once per subdomain with the table object's nt, dt, wh_filter, cs, sn set to that subdomain's
grid, and adds the results up (a subdomain writes its own trace slots only, and its own share of y).  `time_grid` restates a
grid of r * nt steps with the scalar loops of tests/ddh_general.tables (math.cos / math.sin: numpy's vectorised functions may
differ in the last bit).
"""
from __future__ import annotations

import functools
import math

import numpy as np


def time_grid(omega: float, nt: int, real):
    """(dt, filter, cs, sn) of the grid of nt steps per period 2 pi / omega"""
    T = 2 * math.pi / omega
    dt = T / nt
    filt = np.zeros(nt + 1, dtype=real)
    for k in range(nt + 1):
        filt[k] = dt * (omega / math.pi) * (math.cos(omega * k * dt) - 0.25)
    filt[0] = real(filt[0] * 0.5)
    filt[nt] = real(filt[nt] * 0.5)
    cs = np.zeros(2 * nt + 1, dtype=real)
    sn = np.zeros(2 * nt + 1, dtype=real)
    for k in range(2 * nt + 1):
        t = 0.5 * k * dt
        cs[k] = -math.cos(omega * t)
        sn[k] = math.sin(omega * t)
    return dt, filt, cs, sn


def coefficient_ratios(t, h_a) -> np.ndarray:
    """the `coefficient` rule on the oracle's tables: max(1, ceil((1 - 1e-9) / min a over the subdomain's dofs)), through gI"""
    out = np.zeros(t.n_domains, dtype=np.int32)
    for s in range(t.n_domains):
        a_min = float(np.min(np.asarray(h_a, dtype=np.float64)[t.gI[: int(t.s_dof[s]), s]]))
        out[s] = max(1, math.ceil((1.0 / a_min) * (1.0 - 1e-9)))
    return out


class PerSubdomainOracle:
    """O (oracle.DDH or ddh_general.OracleDDH) with subdomain s on the grid of ratios[s] * O.t.nt steps; O is left as it was"""

    def __init__(self, O, ratios):
        self.O, self.t, self.real, self.size = O, O.t, O.real, O.size
        self.ratios = np.asarray(ratios, dtype=np.int64)
        assert self.ratios.shape == (O.t.n_domains,) and self.ratios.min() >= 1
        self.nt0 = O.t.nt
        self.grids = {int(r): time_grid(O.t.omega, int(r) * self.nt0, O.real) for r in np.unique(self.ratios)}

    def solve(self, x=None, want_y=False, lam=None, want_update=True):
        t = self.t
        keep = (t.nt, t.dt, t.wh_filter, t.cs, t.sn)
        y = upd = None
        try:
            for s in range(t.n_domains):
                r = int(self.ratios[s])
                t.nt = r * self.nt0
                t.dt, t.wh_filter, t.cs, t.sn = self.grids[r]
                ys, us = self.O.solve(x=x, want_y=want_y, lam=lam, want_update=want_update, d0=s, d1=s + 1)
                y = ys if y is None or ys is None else y + ys
                upd = us if upd is None or us is None else upd + us
        finally:
            t.nt, t.dt, t.wh_filter, t.cs, t.sn = keep
        return y, upd

    def rhs(self, f):
        return self.solve(x=f)[1]

    def action(self, lam):
        lam = np.asarray(lam, dtype=self.real)
        upd = self.solve(lam=lam)[1]
        return (self.real(1) * lam + self.real(-1) * upd).astype(self.real)

    def postprocess(self, lam, f):
        return self.solve(x=f, want_y=True, lam=lam, want_update=False)[0]


# ---- a small heterogeneous problem (the physics test and profiles/tools/ddh_time_grid_oracle_flow.py)
def smooth_coefficient(x, y):
    """a from 0.4 at x = -1 to 1 at x = 1: wave speeds 2.5 to 1, `coefficient` ratios 3 (x < 0) and 2 (x > 0) for blocks that meet at x = 0"""
    return 0.4 + 0.3 * (x + 1.0) + 0.0 * y


@functools.lru_cache(maxsize=None)
def physics_case(nx=8, block=4, nb=4):
    """(discretization, omega, h_a, load, labels, n_domains, fp64 OracleDDH, its `coefficient` ratios) on [-1,1]^2, omega = 2 pi nx / 10"""
    import ddh_general as dg
    import oracle

    omega = 2 * math.pi * nx / 10
    d = oracle.Discretization(oracle.Mesh.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), nb)
    h_a = d.nodal(smooth_coefficient)
    f = np.concatenate([oracle.linear_functional(d, oracle.gaussians(omega)), 0.1 * oracle.linear_functional(d, oracle.mass_poly)])
    i, j = np.meshgrid(np.arange(nx), np.arange(nx), indexing="xy")
    labels = ((i // block) + (nx // block) * (j // block)).reshape(-1).astype(np.int32)
    n_domains = (nx // block) ** 2
    O = dg.OracleDDH(d, n_domains, labels, omega, h_a, np.float64)
    return d, omega, h_a, f, labels, n_domains, O, coefficient_ratios(O.t, h_a)


# ---- the stability evidence of DESIGN 5.2, shared by the CPU and the GPU test (computed once per session)
STABILITY_STEPS = 3


@functools.lru_cache(maxsize=None)
def stability_window():
    """config 3's disk window of tests/test_baseline_regime.py, 8 x 8 elements: its fp64 oracle and its `coefficient` ratios"""
    from test_baseline_regime import Window

    w = Window("config3_512_16pi", "disk", nw=8)
    O = w.oracle_ddh(np.float64)
    return w, O, coefficient_ratios(O.t, w.h_a)


@functools.lru_cache(maxsize=None)
def stability_growth_per_subdomain():
    """|T^k v| / |T^(k-1) v| of the per-subdomain oracle on that window (power_iteration, seed 1, STABILITY_STEPS steps)"""
    from test_baseline_regime import power_iteration

    _, O, ratios = stability_window()
    P = PerSubdomainOracle(O, ratios)
    return tuple(power_iteration(lambda v: P.solve(lam=v)[1], O.size, STABILITY_STEPS, seed=1))
