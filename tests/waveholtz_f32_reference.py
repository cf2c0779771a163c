"""The fp32 march of cd.WaveHoltz(..., sweep="lattice", precision="f32"), restated in numpy (TEST INFRASTRUCTURE).

`Model32` is waveholtz_reference.Model with `period` in np.float32: K, invm, Hi, filt, cs, sn, dt, dt / 2 and dt / 6 are each
rounded once from their float64 values (dt / 6 from the double quotient), z and f are rounded on the way in, every intermediate
of the march is float32 (asserted), and the result is returned as float64.  There are no fused multiply-adds and K p is summed in
the order of the stored matrix, so this is A correct fp32 march, not the device's: two correct fp32 marches differ from each other
about as much as each differs from the float64 one.  action, rhs, solution and gmres are the float64 model's on this period
(y = x - S x is formed in float64, as the product does).
"""
from __future__ import annotations

import numpy as np

import waveholtz_reference as wr

F32 = np.float32


def _f32(*xs):
    for x in xs:
        assert x.dtype == F32, x.dtype
    return xs[0] if len(xs) == 1 else xs


class Model32(wr.Model):
    def __init__(self, K, m, h, a, omega, nt, scheme="rk2"):
        super().__init__(K, m, h, a, omega, nt, scheme)
        self.K32 = self.K.astype(F32)
        self.invm32, self.Hi32 = self.invm.astype(F32), self.Hi.astype(F32)
        self.filt32, self.cs32, self.sn32 = (np.asarray(t, dtype=np.float64).astype(F32) for t in (self.filt, self.cs, self.sn))
        self.dt32, self.half_dt32, self.sixth_dt32 = F32(self.dt), F32(0.5 * self.dt), F32(self.dt / 6.0)

    @classmethod
    def of(cls, M: wr.Model) -> "Model32":
        """the fp32 restatement of a float64 model"""
        return cls(M.Kd, M.m, M.h, M.a, M.omega, M.nt, M.scheme)

    def period(self, z=None, f=None):
        n, K, invm, Hi, filt, cs, sn = self.n, self.K32, self.invm32, self.Hi32, self.filt32, self.cs32, self.sn32
        dt, half_dt, sixth, two = self.dt32, self.half_dt32, self.sixth_dt32, F32(2.0)
        z = np.zeros(2 * n, dtype=F32) if z is None else np.asarray(z, dtype=np.float64).astype(F32)
        F, G = (np.zeros(n, dtype=F32),) * 2 if f is None else (np.asarray(f[:n], dtype=np.float64).astype(F32),
                                                                 np.asarray(f[n:], dtype=np.float64).astype(F32))
        _f32(K.data, invm, Hi, filt, cs, sn, z, F, G)
        assert all(type(s) is F32 for s in (dt, half_dt, sixth, two))

        def fq(k, p, q):
            return _f32(invm * _f32(_f32(_f32(K @ p) - _f32(Hi * q)) + _f32(cs[k] * F) + _f32(sn[k] * G)))

        p, q = z[:n].copy(), z[n:].copy()
        u, v = _f32(filt[0] * p, filt[0] * q)
        for it in range(1, self.nt + 1):
            if self.scheme == "rk2":
                qh = q + half_dt * fq(2 * it - 2, p, q)
                ph = p - half_dt * q
                p = p - dt * qh
                q = q + dt * fq(2 * it - 1, ph, qh)
                _f32(qh, ph)
            else:
                k1p, k1q = -q, fq(2 * it - 2, p, q)
                p2, q2 = p + half_dt * k1p, q + half_dt * k1q
                k2p, k2q = -q2, fq(2 * it - 1, p2, q2)
                p3, q3 = p + half_dt * k2p, q + half_dt * k2q
                k3p, k3q = -q3, fq(2 * it - 1, p3, q3)
                p4, q4 = p + dt * k3p, q + dt * k3q
                k4p, k4q = -q4, fq(2 * it, p4, q4)
                _f32(p2, q2, p3, q3, p4, q4)
                p = p + sixth * _f32(k1p + two * k2p + two * k3p + k4p)
                q = q + sixth * _f32(k1q + two * k2q + two * k3q + k4q)
            u = u + filt[it] * p
            v = v + filt[it] * q
            _f32(p, q, u, v)
        return np.concatenate([u, v]).astype(np.float64)
