"""DDH local solves with a selectable integrator, restated in numpy (TEST INFRASTRUCTURE).

The oracle's local solve (oracle/ddh_body.inc) is the reference's: explicit midpoint rule (RK2) on one grid.  `Restatement`
restates rhs / action / postprocess for block decompositions on the tables of ddh_general.OracleDDH with the scheme as a
parameter ("rk2" or "rk4", DESIGN 4.3 "Runge-Kutta 4"), every subdomain on a grid of its own, in float64 or float32:

  * per subdomain the dense stiffness S_s, assembled from ddh_general.element_stiffness through sI;
  * coefficients and sources as the kernels' load_dof: invm = 1 / (a^2 m), F, Gf = x (+ H lambda on the trace dofs), Hi = H a;
  * the march: wh_iters x (restart p = u, q = v, u *= filt[0], v *= filt[0]; nt steps; u += filt[it] p, v += filt[it] q after
    step it), with y = (p, q), f(t; p, q) = (-q, invm (S p - Hi q + c(t) F + s(t) Gf)) and c, s = cs, sn at the half steps:
      rk2:  qh = q + dt/2 f_q(t[2it-2]; p, q),  ph = p - dt/2 q,  p -= dt qh,  q += dt f_q(t[2it-1]; ph, qh)
      rk4:  k1 = f(t[2it-2]; y), k2 = f(t[2it-1]; y + dt/2 k1), k3 = f(t[2it-1]; y + dt/2 k2), k4 = f(t[2it]; y + dt k3),
            y += dt/6 (k1 + 2 k2 + 2 k3 + k4);
  * outputs as publish_dof: v /= omega, y += m gmi (u, v), update = -lambda -+ 2 a omega (v, u) through B.

Subdomain s marches ratios[s] * nt_base steps, nt_base = ceil(nt_mesh / coarsen); its (dt, filter, cs, sn) come from
ddh_time_grids.time_grid.  In "rk2" mode the restatement is pinned against ddh_time_grids.PerSubdomainOracle
(tests/test_ddh_rk4.py) before anything relies on it.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import ddh_general as dg
import ddh_time_grids as tg


def base_steps(nt_mesh: int, coarsen: int) -> int:
    return -(-int(nt_mesh) // int(coarsen))


class Restatement:
    """O: ddh_general.OracleDDH (its tables and geometric factors are read, nothing is changed)"""

    def __init__(self, O, scheme="rk4", ratios=None, coarsen=1, real=None, wh_iters=5):
        assert scheme in ("rk2", "rk4")
        t = self.t = O.t
        self.O, self.scheme, self.wh_iters = O, scheme, wh_iters
        self.real = real = O.real if real is None else real
        self.size, self.ndof = O.size, O.d.ndof
        self.ratios = np.ones(t.n_domains, dtype=np.int64) if ratios is None else np.asarray(ratios, dtype=np.int64)
        assert self.ratios.shape == (t.n_domains,) and self.ratios.min() >= 1
        self.nt_base = base_steps(t.nt, coarsen)
        self.grids = {int(r): tg.time_grid(t.omega, int(r) * self.nt_base, real) for r in np.unique(self.ratios)}
        nodes = t.nb * t.nb
        D = np.asarray(t.D, dtype=real).astype(np.float64)
        self.S = []
        for s in range(t.n_domains):
            n = int(t.s_dof[s])
            S = np.zeros((n, n))
            for el in range(int(t.s_elems[s])):
                idx = t.sI[:, :, el, s].reshape(-1, order="F")
                g = np.asarray(O.G[:, el * nodes:(el + 1) * nodes, s], dtype=real).astype(np.float64)
                S[np.ix_(idx, idx)] += dg.element_stiffness(D, g)
            self.S.append(S.astype(real))

    # ---- one local solve
    def _march(self, s, invm, Hi, F, Gf):
        real = self.real
        S = self.S[s]
        dt, filt, cs, sn = self.grids[int(self.ratios[s])]
        nt = len(filt) - 1
        dt, half = real(dt), real(0.5)
        u, v = np.zeros_like(F), np.zeros_like(F)

        def fq(k, p, q):
            return invm * ((S @ p - Hi * q) + cs[k] * F + sn[k] * Gf)

        for _ in range(self.wh_iters):
            p, q = u.copy(), v.copy()
            u *= filt[0]
            v *= filt[0]
            for it in range(1, nt + 1):
                if self.scheme == "rk2":
                    qh = q + half * dt * fq(2 * it - 2, p, q)
                    ph = p - half * dt * q
                    p = p - dt * qh
                    q = q + dt * fq(2 * it - 1, ph, qh)
                else:
                    k1p, k1q = -q, fq(2 * it - 2, p, q)
                    p2, q2 = p + half * dt * k1p, q + half * dt * k1q
                    k2p, k2q = -q2, fq(2 * it - 1, p2, q2)
                    p3, q3 = p + half * dt * k2p, q + half * dt * k2q
                    k3p, k3q = -q3, fq(2 * it - 1, p3, q3)
                    p4, q4 = p + dt * k3p, q + dt * k3q
                    k4p, k4q = -q4, fq(2 * it, p4, q4)
                    sixth = dt / real(6)
                    p = p + sixth * (k1p + real(2) * k2p + real(2) * k3p + k4p)
                    q = q + sixth * (k1q + real(2) * k2q + real(2) * k3q + k4q)
                u += filt[it] * p
                v += filt[it] * q
        return u, v

    def solve_many(self, inputs):
        """inputs: (x, lam, want_y, want_update) per solve, x / lam None or arrays; one march per subdomain carries all of them as
        columns.  Returns [(y, update)] like oracle.DDH.solve (y float64 2 ndof, update `real` 2 n_lambda; None where not wanted)."""
        t, real = self.t, self.real
        nl, ndof, K = t.n_lambda, self.ndof, len(inputs)
        lams = [None if lam is None else np.asarray(lam, dtype=real) for _, lam, _, _ in inputs]
        ys = [np.zeros(2 * ndof) if wy else None for _, _, wy, _ in inputs]
        upds = [np.zeros(2 * nl, dtype=real) if wu else None for _, _, _, wu in inputs]
        omega = real(t.omega)
        with np.errstate(all="ignore"):  # a march outside the stable range overflows, as on the device
            for s in range(t.n_domains):
                n, nf = int(t.s_dof[s]), int(t.s_fdof[s])
                a = np.asarray(t.a[:n, s], dtype=real)
                m = np.asarray(t.m[:n, s], dtype=real)
                gI = t.gI[:n, s]
                invm = (real(1) / (a * a * m))[:, None]
                F, Gf, Hi = np.zeros((n, K), dtype=real), np.zeros((n, K), dtype=real), np.zeros((n, 1), dtype=real)
                H = np.asarray(t.H[:nf, s], dtype=real)
                rd, wr = t.B[:nf, 0, s], t.B[:nf, 1, s]
                l_rd, m_rd = np.zeros((nf, K), dtype=real), np.zeros((nf, K), dtype=real)
                for k, ((x, _, _, _), lam) in enumerate(zip(inputs, lams)):
                    if x is not None:
                        F[:, k] = np.asarray(x[gI], dtype=real)
                        Gf[:, k] = np.asarray(x[ndof + gI], dtype=real)
                    if lam is not None:
                        has = rd >= 0
                        l_rd[has, k] = lam[rd[has]]
                        m_rd[has, k] = lam[nl + rd[has]]
                        F[:nf, k] += H * l_rd[:, k]
                        Gf[:nf, k] += H * m_rd[:, k]
                Hi[:nf, 0] = H * a[:nf]
                u, v = self._march(s, invm, Hi, F, Gf)
                v = v * (real(1) / omega)
                M = m * np.asarray(t.gmi[:n, s], dtype=real)
                has = wr >= 0
                Sc = real(2) * a[:nf] * omega
                for k in range(K):
                    if ys[k] is not None:
                        np.add.at(ys[k], gI, (M * u[:, k]).astype(np.float64))
                        np.add.at(ys[k], ndof + gI, (M * v[:, k]).astype(np.float64))
                    if upds[k] is not None:
                        upds[k][wr[has]] = (-l_rd[:, k] - Sc * v[:nf, k])[has]
                        upds[k][nl + wr[has]] = (-m_rd[:, k] + Sc * u[:nf, k])[has]
        return list(zip(ys, upds))

    def solve(self, x=None, want_y=False, lam=None, want_update=True):
        return self.solve_many([(x, lam, want_y, want_update)])[0]

    def rhs(self, f):
        return self.solve(x=f)[1]

    def action(self, lam):
        lam = np.asarray(lam, dtype=self.real)
        return (lam - self.solve(lam=lam)[1]).astype(self.real)

    def postprocess(self, lam, f):
        return self.solve(x=f, want_y=True, lam=lam, want_update=False)[0]

    def outputs(self, f, lam):
        """(rhs(f), action(lam), postprocess(lam, f)) from one march per subdomain"""
        lam = np.asarray(lam, dtype=self.real)
        (_, b), (_, upd), (u, _) = self.solve_many([(f, None, False, True), (None, lam, False, True), (f, lam, True, False)])
        return b, (lam - upd).astype(self.real), u


# ---- the sweep shapes of tests/test_gpu_ddh_time_grids.py, shared by the CPU and the GPU tests (every reference computed once)
NX, NB_SWEEP = 16, 4
REALS = {"f64": np.float64, "f32": np.float32}


class SweepCase:
    """16 x 16 elements on [-1,1]^2, n_basis 4, a == 1, omega = 2 pi 16 / 10 (nt_mesh about 800), blocks of `block`: the inputs
    of tests/test_gpu_ddh_time_grids.Case and the fp64 / fp32 tables; nothing in it is changed after construction"""

    def __init__(self, block):
        import oracle

        self.block, self.omega = block, 2 * math.pi * NX / 10
        self.d = d = oracle.Discretization(oracle.Mesh.uniform_rect(NX, -1.0, 1.0, NX, -1.0, 1.0), NB_SWEEP)
        self.h_a = np.ones(d.ndof)
        self.fh = np.concatenate([oracle.linear_functional(d, oracle.gaussians(self.omega)), 0.1 * oracle.linear_functional(d, oracle.mass_poly)])
        self.n_domains = (NX // block) ** 2
        i, j = np.meshgrid(np.arange(NX), np.arange(NX), indexing="xy")
        self.labels = ((i // block) + (NX // block) * (j // block)).reshape(-1).astype(np.int32)
        self.O = {name: dg.OracleDDH(d, self.n_domains, self.labels, self.omega, self.h_a, real) for name, real in REALS.items()}
        O = self.O["f64"]
        self.nt_mesh, self.size = O.t.nt, O.size
        n, B = O.size, O.t.B
        lam = np.random.default_rng(7).standard_normal(n)
        used = np.unique(B[B >= 0])
        lam[np.setdiff1d(np.arange(n), np.concatenate([used, used + O.t.n_lambda]))] = 0.0
        self.lam = lam
        written = np.unique(B[:, 1, :][B[:, 1, :] >= 0])
        self.written = np.concatenate([written, written + O.t.n_lambda])


@functools.lru_cache(maxsize=None)
def sweep_case(block=4):
    return SweepCase(block)


@functools.lru_cache(maxsize=None)
def sweep_outputs(block, scheme, coarsen, ratios=None, precision="f64", refine=1):
    """(rhs, action on the written slots, postprocess) of the restatement on sweep_case(block); ratios: a tuple or None (all 1);
    refine: the base grid has `refine` times the mesh grid's steps (a finer reference)"""
    c = sweep_case(block)
    r = np.ones(c.n_domains, dtype=np.int64) if ratios is None else np.asarray(ratios, dtype=np.int64)
    R = Restatement(c.O[precision], scheme, r * refine, coarsen)
    b, y, u = R.outputs(c.fh, c.lam)
    return b, y[c.written], u


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) / np.linalg.norm(np.asarray(b, dtype=np.float64)))


@functools.lru_cache(maxsize=None)
def stability_growth_rk4(coarsen):
    """|T^k v| / |T^(k-1) v| of the rk4 restatement on ddh_time_grids.stability_window (config 3's disk window, nt_mesh 5120), all
    ratios 1, base grid coarsened by `coarsen` (power_iteration, seed 1, STABILITY_STEPS steps)"""
    from test_baseline_regime import power_iteration

    w, O, _ = tg.stability_window()
    R = Restatement(O, "rk4", None, coarsen)
    return tuple(power_iteration(lambda v: R.solve(lam=v)[1], O.size, tg.STABILITY_STEPS, seed=1))
