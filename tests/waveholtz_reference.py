"""Whole-domain WaveHoltz, restated in numpy on dense matrices (TEST INFRASTRUCTURE).

The discrete problem is (K - w^2 M + i w H) U = f with M = diag(a^2 m), m the Gauss-Lobatto lumped mass, and H = diag(a h), h the
lumped face mass of the absorbing faces (zero elsewhere).  `Model.period(z, f)` is W(z; f): one filtered period of the march of
tests/ddh_rk.py (module docstring and Restatement._march, the same expressions in the same order) with a dense global K in the
place of the subdomain's S and z = [u; v]:
    p = u, q = v;  u *= filt[0], v *= filt[0];  nt steps of rk2 / rk4;  u += filt[it] p, v += filt[it] q after step it,
    f_q(k; p, q) = invm (K p - Hi q + cs[k] F + sn[k] G),  invm = 1 / (a^2 m),  Hi = h a,  (F, G) = (f_re, f_im).
W(z; f) = S z + W(0; f); the fixed point solves (I - S) z = W(0; f) and U = u + i v / w.

K comes from the pinned restatements: `collocated_stiffness` assembles the n_basis-point Gauss-Lobatto stiffness as
ddh_rk.Restatement does on the tables of one subdomain that covers the mesh; `gauss_stiffness` builds the n_basis + 1 point
Gauss-Legendre one column by column from the oracle's stiffness apply.  Everything is float64 and computed once per case.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import ddh_general as dg
import ddh_rk
import ddh_time_grids as tg
import oracle


def mesh_steps(omega: float, min_h: float, nb: int) -> int:
    """steps of the mesh grid, the expression of ddh_general.tables"""
    T = 2 * math.pi / omega
    return int(math.ceil(T / (0.2 * 0.5 * min_h / (nb * nb))))


def period_steps(omega, min_h, nb, coarsen=1, ratio=1) -> int:
    return int(ratio) * ddh_rk.base_steps(mesh_steps(omega, min_h, nb), coarsen)


def coefficient_ratio(h_a) -> int:
    return max(1, int(math.ceil((1.0 / float(np.min(h_a))) * (1.0 - 1e-9))))


def one_subdomain(disc, omega, h_a):
    """ddh_general.OracleDDH on one subdomain that covers the mesh (fp64): its tables carry m, H, a and the renumbering"""
    return dg.OracleDDH(disc, 1, np.zeros(disc.mesh.n_elem, dtype=np.int32), omega, h_a, np.float64)


def collocated_stiffness(O) -> np.ndarray:
    """dense global K of the collocated rule: Restatement's S of the one subdomain, back in the global numbering"""
    S = ddh_rk.Restatement(O, "rk2").S[0]
    n = O.d.ndof
    gI = O.t.gI[:n, 0]
    K = np.zeros((n, n))
    K[np.ix_(gI, gI)] = S
    return K


def gauss_stiffness(disc) -> np.ndarray:
    """dense global K of the n_basis + 1 point Gauss-Legendre rule, column by column from the oracle's apply"""
    St = oracle.Stiffness(disc)
    n = disc.ndof
    K = np.zeros((n, n))
    e = np.zeros(n)
    for j in range(n):
        e[j] = 1.0
        K[:, j] = St.apply(e)
        e[j] = 0.0
    return K


def lumped(disc, faces=None):
    """(m, h): Gauss-Lobatto lumped mass, and lumped face mass of `faces` (None: every boundary edge) as an H1 vector"""
    m = 1.0 / oracle.diag_inv_mass(disc)
    fs = oracle.FaceSpaceO(disc, list(disc.mesh.boundary_edges if faces is None else faces))
    h = np.zeros(disc.ndof)
    h[fs.proj] = 1.0 / oracle.diag_inv_facemass(fs)
    return m, h


class Model:
    """W(z; f) for dense K, lumped m and h, nodal a; scheme "rk2" or "rk4" on a grid of nt steps"""

    def __init__(self, K, m, h, a, omega, nt, scheme="rk2"):
        assert scheme in ("rk2", "rk4")
        import scipy.sparse

        self.Kd, self.omega, self.nt, self.scheme = np.asarray(K, dtype=np.float64), float(omega), int(nt), scheme
        self.K = scipy.sparse.csr_matrix(self.Kd)  # the march multiplies by the stored entries only: a step is then cheap in numpy too
        self.n = n = self.Kd.shape[0]
        a = np.asarray(a, dtype=np.float64)
        self.m, self.h, self.a = np.asarray(m, dtype=np.float64), np.asarray(h, dtype=np.float64), a
        self.invm = 1.0 / (a * a * self.m)
        self.Hi = self.h * a
        self.dt, self.filt, self.cs, self.sn = tg.time_grid(self.omega, self.nt, np.float64)
        assert a.shape == self.m.shape == self.h.shape == (n,)

    def period(self, z=None, f=None):
        n, K, invm, Hi, dt, filt, cs, sn = self.n, self.K, self.invm, self.Hi, self.dt, self.filt, self.cs, self.sn
        z = np.zeros(2 * n) if z is None else np.asarray(z, dtype=np.float64)
        F, G = (np.zeros(n), np.zeros(n)) if f is None else (np.asarray(f[:n], dtype=np.float64), np.asarray(f[n:], dtype=np.float64))
        u, v = z[:n].copy(), z[n:].copy()
        half = 0.5

        def fq(k, p, q):
            return invm * ((K @ p - Hi * q) + cs[k] * F + sn[k] * G)

        p, q = u.copy(), v.copy()
        u *= filt[0]
        v *= filt[0]
        for it in range(1, self.nt + 1):
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
                sixth = dt / 6.0
                p = p + sixth * (k1p + 2.0 * k2p + 2.0 * k3p + k4p)
                q = q + sixth * (k1q + 2.0 * k2q + 2.0 * k3q + k4q)
            u += filt[it] * p
            v += filt[it] * q
        return np.concatenate([u, v])

    def rhs(self, f):
        return self.period(None, f)

    def action(self, x):
        x = np.asarray(x, dtype=np.float64)
        return x - self.period(x, None)

    def solution(self, z):
        return np.concatenate([z[: self.n], z[self.n:] / self.omega])

    def iterate(self, f, periods):
        """`periods` periods from zero under f: what DDH's local solve does with one subdomain"""
        z = np.zeros(2 * self.n)
        for _ in range(periods):
            z = self.period(z, f)
        return z

    def direct(self, f):
        """[Re U; Im U] of the direct solve of (K - w^2 M + i w H) U = f_re + i f_im"""
        w, n = self.omega, self.n
        A = self.Kd.astype(np.complex128) + np.diag(-w * w * self.a * self.a * self.m + 1j * w * self.a * self.h)
        U = np.linalg.solve(A, f[:n] + 1j * f[n:])
        return np.concatenate([U.real, U.imag])

    def gmres(self, f, m, maxit, tol, orth="mgs"):
        """(z, info) of lgmres_ref at k = 0 on (I - S) z = W(0; f), from zero"""
        import lgmres_reference as lr

        return lr.lgmres_ref(self.action, self.rhs(f), m, maxit, tol, 0, orth=orth)


def rel(a, b) -> float:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def example_load(disc, omega):
    """the examples' Gaussians in the real part and 0.1 mass_poly in the imaginary part (ddh_rk.SweepCase's load)"""
    return np.concatenate([oracle.linear_functional(disc, oracle.gaussians(omega)), 0.1 * oracle.linear_functional(disc, oracle.mass_poly)])


def smooth_coefficient(disc):
    """a smooth a in [0.6, 1]"""
    xy = disc.coordinates()
    return 0.8 + 0.2 * np.sin(2.0 * xy[0] + 0.3) * np.cos(1.5 * xy[1] - 0.2)


class Case:
    """One mesh, basis and frequency with a load and a coefficient; K, m, h are built on request and kept.  Nothing in it is
    changed after construction."""

    def __init__(self, disc, omega, h_a=None, faces=None):
        self.d, self.omega, self.faces = disc, float(omega), faces
        self.h_a = np.ones(disc.ndof) if h_a is None else np.asarray(h_a, dtype=np.float64)
        self.f = example_load(disc, omega)
        self.min_h = disc.mesh.min_h()

    @functools.cached_property
    def O(self):
        return one_subdomain(self.d, self.omega, self.h_a)

    @functools.cached_property
    def mh(self):
        return lumped(self.d, self.faces)

    @functools.cached_property
    def mh_tables(self):
        """(m, h) as the tables of the one subdomain carry them (face-first numbering), back through gI: every boundary edge"""
        t, n = self.O.t, self.d.ndof
        gI = t.gI[:n, 0]
        m, h = np.zeros(n), np.zeros(n)
        m[gI] = t.m[:n, 0]
        nf = int(t.s_fdof[0])
        h[gI[:nf]] = t.H[:nf, 0]
        return m, h

    @functools.cached_property
    def K_lobatto(self):
        return collocated_stiffness(self.O)

    @functools.cached_property
    def K_gauss(self):
        return gauss_stiffness(self.d)

    def nt(self, coarsen=1, ratio=1):
        return period_steps(self.omega, self.min_h, self.d.nb, coarsen, ratio)

    @functools.lru_cache(maxsize=None)
    def model(self, scheme="rk2", coarsen=1, ratio=1, stiffness="lobatto"):
        m, h = self.mh
        return Model(self.K_lobatto if stiffness == "lobatto" else self.K_gauss, m, h, self.h_a, self.omega, self.nt(coarsen, ratio), scheme)


@functools.lru_cache(maxsize=None)
def uniform_case(nx, nb, smooth=False):
    """[-1, 1]^2 in nx x nx elements, omega = 2 pi nx / 10; a == 1 or smooth_coefficient"""
    d = oracle.Discretization(oracle.Mesh.uniform_rect(nx, -1.0, 1.0, nx, -1.0, 1.0), nb)
    return Case(d, 2 * math.pi * nx / 10, smooth_coefficient(d) if smooth else None)
