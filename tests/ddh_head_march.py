"""numpy restatements of the step schedules of DDH kernel 5's scaled march (march 2) on one subdomain of 4 x 4 elements, n_basis 4:
the one that multiplies the head of the first sweep's chain out in every step (head 1, wh_march_pairs_scaled) and the one that
carries the product (head 2, wh_march_pairs_carried), csrc/kernels/ddh_element_lane.hpp.  A helper, no test; no GPU.

The subdomain is held as the kernel holds it: one row per element, 16 node values each, so a node that m elements share exists in
m copies, and the assembly sums the copies' chains and hands the one sum to all of them.  The element operator is the separable
one, z'(k, l) = Dg w + sum Bx(k, j) w(j, l) + sum By(l, j) w(k, j) with the node weight W folded into the per-dof constants.  What
is restated is the schedule, which value is multiplied by which coefficient and where a rounding falls on the state; the order
inside a chain is the element's node order, the same for both schedules, with the head as the chain's first term.  Every array
has the dtype asked for and no scalar of another precision enters a product.
"""
import numpy as np

NB, NEL = 4, 4
SIDE = NEL * (NB - 1) + 1  # nodes a side of the subdomain
INTERIOR = [k + NB * l for l in (1, 2) for k in (1, 2)]  # element-interior nodes: Hi = 0, one copy


def gll4():
    x = np.array([-1.0, -1.0 / np.sqrt(5.0), 1.0 / np.sqrt(5.0), 1.0])
    w = np.array([1.0, 5.0, 5.0, 1.0]) / 6.0
    D = np.zeros((NB, NB))
    for i in range(NB):
        for j in range(NB):
            if i != j:
                D[i, j] = np.prod([(x[i] - x[m]) / (x[j] - x[m]) for m in range(NB) if m not in (i, j)]) / (x[j] - x[i])
        D[i, i] = -D[i].sum()
    return x, w, D


def case(hx=0.25, hy=0.25, omega=6.0, nt=400, wh_iters=5, seed=5):
    """A subdomain problem in fp64: the folded element tables, the per-copy constants and the time grid.  Stable: asserted."""
    _, w, D = gll4()
    A1 = D.T @ np.diag(w) @ D
    gam, bet = w * hx / 2, w * hy / 2                     # 1D masses
    Ax, Ay = A1 * (2 / hx), A1 * (2 / hy)
    Bx, By = Ax / gam[:, None], Ay / bet[:, None]          # W = gam_k bet_l factored out
    K = np.zeros((NB * NB, NB * NB))                       # z' = K w on one element
    for l in range(NB):
        for k in range(NB):
            for j in range(NB):
                K[k + NB * l, j + NB * l] += Bx[k, j]
                K[k + NB * l, k + NB * j] += By[l, j]
    W = np.array([gam[k] * bet[l] for l in range(NB) for k in range(NB)])
    idx = np.array([[(3 * ex + k) + SIDE * (3 * ey + l) for l in range(NB) for k in range(NB)] for ey in range(NEL) for ex in range(NEL)])
    n = SIDE * SIDE
    mult = np.bincount(idx.ravel(), minlength=n).astype(float)
    rng = np.random.default_rng(seed)
    a = 0.5 + 0.5 * rng.random(n)                          # a coefficient in [0.5, 1]
    mass = np.bincount(idx.ravel(), weights=np.tile(W, NEL * NEL), minlength=n)
    gx, gy = np.arange(n) % SIDE, np.arange(n) // SIDE
    edge = (gx == 0) | (gx == SIDE - 1) | (gy == 0) | (gy == SIDE - 1)
    line = np.where((gx == 0) | (gx == SIDE - 1), 1.0, 0.0) * hy + np.where((gy == 0) | (gy == SIDE - 1), 1.0, 0.0) * hx
    Hi_g = np.where(edge, 0.1 * omega * line / 12.0, 0.0)   # an impedance term on the subdomain's boundary, hm Hi < 0.2 (asserted)
    F_g, G_g = np.where(edge, rng.standard_normal(n), 0.0), np.where(edge, rng.standard_normal(n), 0.0)
    invm_g = 1.0 / (a * mass)
    Wc = np.tile(W, (NEL * NEL, 1))
    c = dict(K=K, idx=idx, n=n, rm=1.0 / mult[idx], invm=Wc * invm_g[idx], Hi=Hi_g[idx] / Wc, F=F_g[idx] / Wc, Gf=G_g[idx] / Wc,
             nt=nt, wh_iters=wh_iters)
    T = 2 * np.pi / omega
    dt = T / nt
    c["dt"] = dt
    t = dt * np.arange(nt + 1)
    filt = (2 / T) * (np.cos(omega * t) - 0.25) * dt
    filt[0] *= 0.5
    filt[-1] *= 0.5
    c["filt"] = filt
    stage = np.stack([t[:-1], t[:-1] + 0.5 * dt], axis=1).ravel()  # the two stage times of every step
    c["cs"], c["sn"] = np.cos(omega * stage), np.sin(omega * stage)
    assert np.all(c["Hi"][:, INTERIOR] == 0) and np.all(c["rm"][:, INTERIOR] == 1)
    assert 0.01 < (0.5 * dt * c["invm"] * c["Hi"]).max() < 0.2  # the damping is there and the explicit step takes it
    # the midpoint rule amplifies a mode of frequency w by 1 + (w dt)^4 / 8 a step: (w dt)^2 < 0.1 keeps a pass within a factor 2
    Kg = np.zeros((n, n))
    for e in range(NEL * NEL):
        Kg[np.ix_(idx[e], idx[e])] += W[:, None] * K
    assert dt * dt * np.abs(np.linalg.eigvals(invm_g[:, None] * Kg)).max() < 0.1
    return c


def _cast(c, dtype):
    return {k: (v.astype(dtype) if isinstance(v, np.ndarray) and v.dtype.kind == "f" else dtype(v) if isinstance(v, float) else v) for k, v in c.items()}


def _assemble(z, idx, n):
    total = np.zeros(n, dtype=z.dtype)
    np.add.at(total, idx, z)
    return total[idx]


def march(c, dtype, carried):
    """(u, v) per node of the subdomain after wh_iters WaveHoltz passes from 0, sources in the first pass only.
    carried False: the state is qs = q / (2 hm), the first chain opens on am qs (wh_march_pairs_scaled);
    carried True:  the state is Y = am qs, the first chain opens on Y, Y = fma(am, z, Y), v = vy c2 (2 / dt) (wh_march_pairs_carried)."""
    c = _cast(c, dtype)
    K, idx, n, rm, dt = c["K"], c["idx"], c["n"], c["rm"], c["dt"]
    one, two, half = dtype(1), dtype(2), dtype(0.5)
    hm = (half * dt) * c["invm"]
    b = hm * c["Hi"]
    cc = dt * hm
    am = (two * (one - b)) * rm
    bm = -b * rm
    c2 = cc / am
    Fm, Gm = c["F"] * rm, c["Gf"] * rm
    inner = np.zeros(16, dtype=bool)
    inner[INTERIOR] = True
    assert np.all(am[:, inner] == two) and np.all(bm[:, inner] == 0)
    Kt = np.ascontiguousarray(K.T)

    def sweep(w, head):
        # the chain opens on the head and takes the products one by one, each rounded onto the accumulator: elementwise numpy, the
        # same on every machine
        acc = head
        for j in range(NB * NB):
            acc = acc + w[:, j:j + 1] * Kt[j]
        return _assemble(acc, idx, n)

    u = np.zeros_like(hm)
    v = np.zeros_like(hm)  # vs, or vy
    r = None
    for whit in range(c["wh_iters"]):
        src = whit == 0
        p, q = u.copy(), v.copy()
        u, v = u * c["filt"][0], v * c["filt"][0]
        for it in range(1, c["nt"] + 1):
            c0, s0, c1, s1 = c["cs"][2 * it - 2], c["sn"][2 * it - 2], c["cs"][2 * it - 1], c["sn"][2 * it - 1]
            kw = c["filt"][it]
            head = q.copy() if carried else am * q
            if src:
                head = s0 * Gm + (c0 * Fm + head)
            ph = p - (c2 if carried else cc) * q
            qt = sweep(p, head)
            p = p - cc * qt
            head = bm * qt
            if src:
                head = s1 * Gm + (c1 * Fm + head)
            z = sweep(ph, head)
            q = am * z + q if carried else q + z
            u = u + kw * p
            v = v + kw * q
        if whit == 0:
            r = (u.copy(), v.copy())
        else:
            u, v = u + r[0], v + r[1]
    v = v * ((c2 if carried else cc) * (two / dt))
    assert u.dtype == dtype and v.dtype == dtype
    # the copies of a node hold one value: return it per node
    out_u, out_v = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
    out_u[idx], out_v[idx] = u, v
    assert np.array_equal(out_u[idx], u) and np.array_equal(out_v[idx], v)
    return out_u, out_v
