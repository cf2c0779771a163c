"""The three-dimensional box problem of cd.WaveHoltzBox, restated in numpy on dense matrices (TEST INFRASTRUCTURE).

Written from the formulas in include/cuddh_hip.h (cuddh_wave_box, cuddh_wave_box_describe): with the product's own 1-D tables
A = D^T diag(w) D and w (cuddh_wave_lattice_tables), assembled along a line of n elements that overlap in one node,
    K = cx Wz (x) Wy (x) Ax + cy Wz (x) Ay (x) Wx + cz Az (x) Wy (x) Wx,   m = (hx hy hz / 8) Wz (x) Wy (x) Wx,
    h = sum of the lumped face masses of the absorbing faces a node lies on,
built by np.kron; node (I, J, K) has index I + Lx (J + Ly K), so the z factor comes first in every product.  The dense K, m and
h feed tests/waveholtz_reference.Model, which knows nothing of dimensions.
"""
from __future__ import annotations

import functools

import numpy as np

FACES = ("x0", "x1", "y0", "y1", "z0", "z1")


@functools.lru_cache(maxsize=None)
def tables(nb):
    """(A, w) of the product: cuddh_wave_lattice_tables"""
    import cuddhelmholtz_amd as cd
    from cuddhelmholtz_amd import _native as N

    A, w = np.zeros((nb, nb)), np.zeros(nb)
    basis = cd.Basis(nb)  # (kept alive over the call)
    assert N.lib.cuddh_wave_lattice_tables(basis._h, A.ctypes.data, w.ctypes.data) == 0, N.last_error()
    A.setflags(write=False)
    w.setflags(write=False)
    return A, w


def line(n, nb):
    """(A^, W) of a line of n elements: the element matrix and the weights added up where elements overlap"""
    A, w = tables(nb)
    H = nb - 1
    L = n * H + 1
    Ah, W = np.zeros((L, L)), np.zeros(L)
    for e in range(n):
        s = slice(e * H, e * H + nb)
        Ah[s, s] += A
        W[s] += w
    return Ah, W


def nodes_1d(a, b, n, nb):
    """the L collocation points of [a, b] in n elements"""
    import cuddhelmholtz_amd as cd

    x, _ = cd.quadrature(nb)
    H, h = nb - 1, (b - a) / n
    out = np.zeros(n * H + 1)
    for e in range(n):
        out[e * H:e * H + nb] = a + h * (e + 0.5 * (x + 1.0))
    return out


def face_mask(absorbing):
    return sum(1 << FACES.index(f) for f in absorbing)


class Box:
    """dense K, m, h of one box; shape = (nx, ny, nz), box = ((ax, bx), (ay, by), (az, bz)); nothing is changed after construction"""

    def __init__(self, shape, box, nb, absorbing=FACES):
        self.shape, self.box, self.nb, self.absorbing = tuple(shape), tuple(map(tuple, box)), nb, tuple(absorbing)
        self.hs = tuple((b - a) / n for (a, b), n in zip(self.box, self.shape))
        self.L = tuple(n * (nb - 1) + 1 for n in self.shape)
        self.n = self.L[0] * self.L[1] * self.L[2]

    @functools.cached_property
    def lines(self):
        return [line(n, self.nb) for n in self.shape]

    @functools.cached_property
    def K(self):
        (Ax, Wx), (Ay, Wy), (Az, Wz) = self.lines
        hx, hy, hz = self.hs
        d = np.diag
        return (hy * hz / (2 * hx) * np.kron(d(Wz), np.kron(d(Wy), Ax)) + hx * hz / (2 * hy) * np.kron(d(Wz), np.kron(Ay, d(Wx)))
                + hx * hy / (2 * hz) * np.kron(Az, np.kron(d(Wy), d(Wx))))

    @functools.cached_property
    def m(self):
        (_, Wx), (_, Wy), (_, Wz) = self.lines
        hx, hy, hz = self.hs
        return hx * hy * hz / 8 * np.kron(Wz, np.kron(Wy, Wx))

    @functools.cached_property
    def h(self):
        (_, Wx), (_, Wy), (_, Wz) = self.lines
        hx, hy, hz = self.hs
        Lx, Ly, Lz = self.L

        def end(L, first):
            e = np.zeros(L)
            e[0 if first else L - 1] = 1.0
            return e

        h = np.zeros(self.n)
        for f in self.absorbing:
            first = f[1] == "0"
            if f[0] == "x":
                h += hy * hz / 4 * np.kron(Wz, np.kron(Wy, end(Lx, first)))
            elif f[0] == "y":
                h += hx * hz / 4 * np.kron(Wz, np.kron(end(Ly, first), Wx))
            else:
                h += hx * hy / 4 * np.kron(end(Lz, first), np.kron(Wy, Wx))
        return h

    @functools.cached_property
    def nodes(self):
        """(Lz, Ly, Lx, 3)"""
        x, y, z = (nodes_1d(a, b, n, self.nb) for (a, b), n in zip(self.box, self.shape))
        out = np.zeros((self.L[2], self.L[1], self.L[0], 3))
        out[..., 0], out[..., 1], out[..., 2] = x[None, None, :], y[None, :, None], z[:, None, None]
        return out

    def nt(self, omega, coarsen=1, ratio=1):
        import waveholtz_reference as wr

        return wr.period_steps(omega, min(self.hs), self.nb, coarsen, ratio)

    def model(self, omega, a, scheme="rk2", coarsen=1, ratio=1):
        import waveholtz_reference as wr

        return wr.Model(self.K, self.m, self.h, np.asarray(a, dtype=np.float64).reshape(-1), omega, self.nt(omega, coarsen, ratio), scheme)

    def smooth_coefficient(self, lo=0.8, hi=1.25):
        """a smooth a whose smallest nodal value is lo and whose largest is hi"""
        X = self.nodes
        s = np.sin(2.0 * X[..., 0] + 0.3) * np.cos(1.5 * X[..., 1] - 0.2) * np.cos(1.1 * X[..., 2] + 0.4)
        a = (lo + (hi - lo) * (s - s.min()) / (s.max() - s.min())).reshape(-1)
        return np.clip(a, lo, hi)

    def example_load(self, omega):
        """[f_re; f_im]: m times a Gaussian in the real part and m times 0.1 of a polynomial in the imaginary part"""
        X = self.nodes.reshape(-1, 3)
        c = np.array([0.5 * (a + b) for a, b in self.box]) + 0.1 * np.array([h for h in self.hs])
        g = np.exp(-omega * omega / 4.0 * np.sum((X - c) ** 2, axis=1))
        poly = 0.1 * (3.0 * X[:, 0] ** 2 - 2.0 * X[:, 0] * X[:, 1] + X[:, 2] + 1.0)
        return np.concatenate([self.m * g, self.m * poly])
