// What every DDH local-solve kernel is built from, part of the one translation unit ddh.hip (which includes this file
// first; ddh_element_lane.hpp stands on it): the launch's arguments DdhArgs, the per-subdomain time grids and the grouped
// rows of kernel 13, the scheme tags, and the local solve around a sweep: load_dof -> wh_march -> publish_dof.  Device
// code and the argument structs only; which kernel a plan runs and how it is launched is in ddh.hip.
#ifndef CUDDH_AMD_DDH_DEVICE_HPP
#define CUDDH_AMD_DDH_DEVICE_HPP

#include "common.hpp"

namespace
{
    template <typename Real>
    struct DdhArgs
    {
        int g_ndof, n_lambda, nt, mx_dof, mx_fdof, nodes, dom_begin, dom_end;
        int wh_iters; // 5 unless a verification run changed it (cuddh_hip_ddh_plan_set_wh_iters)
        int prio;     // != 0: these wavefronts take issue priority over others on their SIMD (cuddh_hip_ddh_plan_set_wave_priority)
        Real omega, dt;
        const int *s_dof, *s_fdof, *B, *gI, *sI;
        const Real *G, *m, *gmi, *a, *H;
        const double *x;
        double *y;
        const Real *lambda;
        Real *update;
        const int *dom_list; // null: positions [dom_begin, dom_end) ARE the subdomains; else subdomain = dom_list[position]
        // general plans (kernels 9, 10): per subdomain, for each dof the element nodes that contribute to it in ascending order,
        // CSR with fixed strides: csr_off (nodes + 1, n_domains), csr_src (nodes, n_domains)
        const int *csr_off, *csr_src;
        int unique_y; // != 0: y entries are written by one subdomain dof each (a vector layout is set): plain adds, no atomics
    };

    template <typename Real>
    __device__ inline int domain_at(const DdhArgs<Real> &A, int position)
    {
        return A.dom_list ? A.dom_list[position] : position;
    }

    // ---------------------------------------------------------------- per-subdomain time grids
    // A plan with time grids (cuddh_hip_ddh_plan_set_time_grids) gives subdomain s the grid grid_of[s]: its own step count and
    // step size and its own filter / cs / sn tables, which lie one grid after the other in the three arrays the kernel is
    // passed.  The kernels that hold ONE subdomain per wavefront or workgroup take a TimeGrids as a last argument (template
    // parameter pack Grids, empty for a plain plan: those instantiations have the arguments and the code they had before).
    // The grid is wave-uniform, but a subdomain located from the wave index looks divergent to the compiler: the grid's index
    // and what is read of it (nt, dt, the two offsets) go through readfirstlane, so that the loop counter, the step sizes and
    // the table bases stay in scalar registers and filt / cs / sn on scalar loads, as on the one grid (without it the time
    // loop gains three vector instructions and its table reads become vector loads).  Wavefronts of one workgroup may run different step counts: the wavefront kernels have no
    // workgroup barriers, and kernel 1's workgroup is one subdomain.
    template <typename Real>
    struct DdhTimeGrid
    {
        int nt, filt_off, cs_off; // steps per period; where the grid's filter (nt + 1) and its cs / sn (2 nt + 1) start
        Real dt;
    };

    template <typename Real>
    struct TimeGrids
    {
        const int *grid_of;             // (n_domains)
        const DdhTimeGrid<Real> *grids; // (n_grids)
    };

    // every launch of a plan with time grids goes through a list (apply: the plan's own where the caller gave none), so the
    // wavefronts need no flag that tells the two cases apart; kernel 11 has no scalar register left for one
    template <typename Real>
    __device__ inline int domain_at(const DdhArgs<Real> &A, int position, const TimeGrids<Real> &)
    {
        return A.dom_list[position];
    }

    template <typename Real>
    struct TimeGridView
    {
        int nt;
        Real dt;
        const Real *filt, *cs, *sn;
    };

    // the grid subdomain s marches on: the launch's one grid ...
    template <typename Real>
    __device__ inline TimeGridView<Real> time_grid_of(const DdhArgs<Real> &A, int, const Real *filt, const Real *cs, const Real *sn)
    {
        return {A.nt, A.dt, filt, cs, sn};
    }

    // the value of a wave-uniform quantity in a scalar register, whatever the compiler can prove about it
    __device__ inline int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
    __device__ inline float wave_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
    __device__ inline double wave_uniform(double v)
    {
        const long long bits = __double_as_longlong(v);
        const int lo = __builtin_amdgcn_readfirstlane(static_cast<int>(bits)), hi = __builtin_amdgcn_readfirstlane(static_cast<int>(bits >> 32));
        return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned int>(lo));
    }

    // ... or its own
    template <typename Real>
    __device__ inline TimeGridView<Real> time_grid_of(const DdhArgs<Real> &, int s, const Real *filt, const Real *cs, const Real *sn,
                                                      const TimeGrids<Real> &TG)
    {
        const DdhTimeGrid<Real> tg = TG.grids[wave_uniform(TG.grid_of[s])];
        const int filt_off = wave_uniform(tg.filt_off), cs_off = wave_uniform(tg.cs_off);
        return {wave_uniform(tg.nt), wave_uniform(tg.dt), filt + filt_off, cs + cs_off, sn + cs_off};
    }

    // ---------------------------------------------------------------- time grids with four subdomains per wavefront (kernel 13)
    // ddh_element_lane_kernel (n_basis 4 and 5) holds a subdomain per 16-lane DPP row and one time grid per march.
    // Its TimeGrids instantiations march once per distinct grid among the wavefront's rows: a pass takes the lowest row
    // not yet published as its leader and that row's grid g; rows on g load, march and publish their own subdomain, every
    // other row takes the leader's (the rule of a launch's tail rows: real data in every row, nothing published).  All that
    // waits through the time loop is one scalar, the mask of the rows that have published: the view below is formed from it
    // at the start of a pass and again behind the march (these kernels have no register to keep it in).
    struct GroupedRows
    {
        int pending, s_lead, g; // rows of the launch still to publish (bit per row, never 0); this pass's leader subdomain and grid
    };

    template <typename Real>
    __device__ inline GroupedRows grouped_rows(const DdhArgs<Real> &A, int s_first, int done, const TimeGrids<Real> &TG)
    {
        GroupedRows R;
        const int rows = A.dom_end - s_first; // >= 1: the wavefront has returned otherwise
        R.pending = wave_uniform((rows >= 4 ? 15 : (1 << rows) - 1) & ~done);
        R.s_lead = wave_uniform(A.dom_list[s_first + __builtin_ctz(R.pending)]);
        R.g = wave_uniform(TG.grid_of[R.s_lead]);
        return R;
    }

    // row `sub` in this pass: active (returns true, s = its own subdomain) or a copy of the leader
    template <typename Real>
    __device__ inline bool grouped_row(const DdhArgs<Real> &A, int s_first, int sub, const GroupedRows &R, const TimeGrids<Real> &TG, int &s)
    {
        bool active = (R.pending >> sub) & 1; // a row of the launch (s_first + sub < A.dom_end) that has not published
        s = R.s_lead;
        if (active)
        {
            const int own = A.dom_list[s_first + sub];
            active = TG.grid_of[own] == R.g;
            if (active)
                s = own;
        }
        return active;
    }

    // the rows that publish in this pass (bit 16 r of the ballot: all lanes of a row agree) and, whatever memory says, the
    // leader, so that every pass ends with fewer rows to go
    __device__ inline int grouped_published(const GroupedRows &R, bool active)
    {
        const unsigned long long b = __builtin_amdgcn_ballot_w64(active);
        return static_cast<int>((b & 1u) | ((b >> 15) & 2u) | ((b >> 30) & 4u) | ((b >> 45) & 8u)) | (R.pending & -R.pending);
    }

    // The launch's arguments read again: from the kernel-argument segment, where a DdhArgs that is the kernel's FIRST
    // parameter starts at offset 0, through a pointer the compiler cannot connect with the one it holds.  A pass reads them
    // before its loads and again behind its march (scalar loads): of the copy the compiler holds, everything a pass needs
    // would wait in scalar registers from before the first pass to the last, through every march, and these kernels have
    // none to spare (spilled to vector lanes they cost the vector registers that decide the occupancy).
    template <typename Real>
    __device__ inline void reread_args(DdhArgs<Real> &L)
    {
        using Segment = const __attribute__((address_space(4))) DdhArgs<Real>;
        Segment *k = (Segment *)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(k));
        __builtin_memcpy(&L, k, sizeof L);
    }

    // threadIdx.x & 63 without threadIdx.x, formed where it is called (the opaque 0 keeps the compiler from forming it once
    // and keeping it): with the wavefront's first position in a scalar register a pass needs nothing else of the thread
    // index, whose vector register is then free through the march
    __device__ inline int lane_here()
    {
        int zero = 0;
        asm volatile("" : "+v"(zero));
        return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, zero));
    }

    template <typename T, typename... Rest>
    __device__ inline const T &first_of(const T &t, const Rest &...) { return t; }

    // ---------------------------------------------------------------- the integrator of a launch
    // A plan with cuddh_hip_ddh_plan_set_integrator(plan, 1) steps with classical RK4.  Its kernels are instantiations of their
    // own: the tag below comes last in the same trailing pack that carries the TimeGrids, so a kernel is instantiated with
    // nothing (RK2, one grid: the code and the symbol it had before), TimeGrids, Rk4Scheme, or TimeGrids then Rk4Scheme.
    struct Rk4Scheme
    {
    };

    template <typename... Opts>
    inline constexpr int scheme_of = 0; // wh_march's SCHEME: 0 RK2, 1 RK4
    template <typename First, typename... Rest>
    inline constexpr int scheme_of<First, Rest...> = scheme_of<Rest...>;
    template <>
    inline constexpr int scheme_of<Rk4Scheme> = 1;

    template <typename Real>
    __device__ inline int domain_at(const DdhArgs<Real> &A, int position, const Rk4Scheme &) { return domain_at(A, position); }
    template <typename Real>
    __device__ inline int domain_at(const DdhArgs<Real> &A, int position, const TimeGrids<Real> &TG, const Rk4Scheme &) { return domain_at(A, position, TG); }
    template <typename Real>
    __device__ inline TimeGridView<Real> time_grid_of(const DdhArgs<Real> &A, int s, const Real *filt, const Real *cs, const Real *sn, const Rk4Scheme &)
    {
        return time_grid_of(A, s, filt, cs, sn);
    }
    template <typename Real>
    __device__ inline TimeGridView<Real> time_grid_of(const DdhArgs<Real> &A, int s, const Real *filt, const Real *cs, const Real *sn,
                                                      const TimeGrids<Real> &TG, const Rk4Scheme &)
    {
        return time_grid_of(A, s, filt, cs, sn, TG);
    }

    // ---------------------------------------------------------------- the local solve around the sweep (shared by all kernels)
    // Coefficients of dof d of subdomain s: invm = 1 / (a^2 m), the sources F, Gf = x (+ H lambda through B on the trace dofs
    // d < fdof), Hi = H a.
    template <typename Real>
    __device__ inline void load_dof(const DdhArgs<Real> &A, int s, int d, int fdof, Real &invm, Real &Hi, Real &F, Real &Gf)
    {
        const size_t dbase = (size_t)A.mx_dof * s, fbase = (size_t)A.mx_fdof * s;
        const Real ai = A.a[dbase + d], mi = A.m[dbase + d];
        invm = Real(1) / (ai * ai * mi);
        Real f = 0, gg = 0, h = 0;
        if (A.x)
        {
            const int gidx = A.gI[dbase + d];
            f = static_cast<Real>(A.x[gidx]);
            gg = static_cast<Real>(A.x[A.g_ndof + gidx]);
        }
        if (d < fdof)
        {
            h = A.H[fbase + d];
            if (A.lambda)
            {
                const int slot = A.B[d + (size_t)A.mx_fdof * (0 + 2 * (size_t)s)];
                if (slot >= 0)
                {
                    f += h * A.lambda[slot];
                    gg += h * A.lambda[A.n_lambda + slot];
                }
            }
            h *= ai;
        }
        F = f;
        Gf = gg;
        Hi = h;
    }

    // The WaveHoltz iterations of one local solve for the N values a lane owns: wh_iters x (restart from the filtered field,
    // nt RK2 steps of size dt with two stiffness sweeps z = S w each, filter accumulation) on the time grid the caller passes
    // (time_grid_of: the launch's, or the subdomain's own).  Returns the filter sums u, v (v not yet
    // divided by omega: publish_dof does that).  -ffp-contract=fast turns the shape of these expressions into FMAs: keep it.
    // LEAN (the matrix-core kernels; 0 is the form every other kernel compiles to, instruction for instruction):
    //   != 0: the step sizes are folded into the per-dof constant (q + (half_dt invm) r instead of q + half_dt (r invm)), one
    //         multiplication less per value and half step, and the values l with bit l of INTERIOR set (value 0 of every lane
    //         in the matrix-core kernels, the four element-interior registers of the element-lane kernel) are known to be no
    //         trace dofs: Hi[l] == 0 and its term is not computed;
    //   1:    their sources F[l], Gf[l] are zero as well (no x given: sources sit on trace dofs only) and are not computed either;
    //   2:    they are kept.
    // SCHEME 1 (scheme_of: a plan with cuddh_hip_ddh_plan_set_integrator(plan, 1)): classical RK4 in place of the midpoint rule.
    //   With y = (p, q) and f(t; p, q) = (-q, invm (S p - Hi q + c(t) F + s(t) Gf)), step it is
    //       k1 = f(t[2 it - 2]; y),  k2 = f(t[2 it - 1]; y + dt/2 k1),  k3 = f(t[2 it - 1]; y + dt/2 k2),  k4 = f(t[2 it]; y + dt k3),
    //       y += dt/6 (k1 + 2 k2 + 2 k3 + k4),
    //   four sweeps per step; restart, filter accumulation and tables are those of RK2 (cs / sn hold every half step).  The
    //   sum of the k is accumulated stage by stage (pa, qa), so a stage's slopes are not kept: per value two registers more than
    //   RK2's loop.  The step size is folded into the per-dof constant in every form (e = (dt invm) r is dt times the slope
    //   of q); LEAN's rules for the INTERIOR values hold as they do for RK2.
    template <int LEAN = 0, unsigned INTERIOR = 1u, int SCHEME = 0, typename Real, int N, typename Sweep>
    __device__ inline void wh_march(const DdhArgs<Real> &A, const int nt, const Real dt, const Real *__restrict__ filt,
                                    const Real *__restrict__ cs, const Real *__restrict__ sn, const Real (&invm)[N], const Real (&Hi)[N], const Real (&F)[N],
                                    const Real (&Gf)[N], Real (&u)[N], Real (&v)[N], Sweep sweep)
    {
        Real p[N], q[N];
#pragma unroll
        for (int l = 0; l < N; ++l)
            p[l] = q[l] = u[l] = v[l] = 0;
        const Real half_dt = Real(0.5) * dt;
        Real hm[N], dm[N]; // LEAN: half_dt invm, dt invm;  RK4: dm alone
        if constexpr (LEAN != 0 || SCHEME == 1)
        {
#pragma unroll
            for (int l = 0; l < N; ++l)
            {
                hm[l] = half_dt * invm[l];
                dm[l] = dt * invm[l];
            }
        }
        for (int whit = 0; whit < A.wh_iters; ++whit)
        {
            {
                const Real k0 = filt[0];
#pragma unroll
                for (int l = 0; l < N; ++l)
                {
                    p[l] = u[l];
                    q[l] = v[l];
                    u[l] *= k0;
                    v[l] *= k0;
                }
            }
            if constexpr (SCHEME == 1)
            {
                const Real sixth = Real(1) / Real(6), third = Real(1) / Real(3);
                const Real sixth_dt = sixth * dt, third_dt = third * dt;
                // r: what invm multiplies in the slope of q, for value l at the stage whose field gave z and whose q is qv
#define CUDDH_RK4_RATE(zv, qv, c, s)                                                                                                              \
    (dm[l] * ((LEAN != 0 && ((INTERIOR >> l) & 1u)) ? (LEAN == 2 ? zv[l] + c * F[l] + s * Gf[l] : zv[l])                                         \
                                                    : (zv[l] - Hi[l] * qv[l]) + c * F[l] + s * Gf[l]))
                for (int it = 1; it <= nt; ++it)
                {
                    const Real c0 = cs[2 * it - 2], s0 = sn[2 * it - 2];
                    const Real c1 = cs[2 * it - 1], s1 = sn[2 * it - 1];
                    const Real c2 = cs[2 * it], s2 = sn[2 * it];
                    const Real kw = filt[it];
                    Real z[N], ps[N], qs[N], pa[N], qa[N];

                    sweep(p, z);
#pragma unroll
                    for (int l = 0; l < N; ++l)
                    {
                        const Real e = CUDDH_RK4_RATE(z, q, c0, s0);
                        pa[l] = p[l] - sixth_dt * q[l];
                        qa[l] = q[l] + sixth * e;
                        ps[l] = p[l] - half_dt * q[l];
                        qs[l] = q[l] + Real(0.5) * e;
                    }
                    sweep(ps, z);
#pragma unroll
                    for (int l = 0; l < N; ++l)
                    {
                        const Real e = CUDDH_RK4_RATE(z, qs, c1, s1);
                        pa[l] -= third_dt * qs[l];
                        qa[l] += third * e;
                        ps[l] = p[l] - half_dt * qs[l];
                        qs[l] = q[l] + Real(0.5) * e;
                    }
                    sweep(ps, z);
#pragma unroll
                    for (int l = 0; l < N; ++l)
                    {
                        const Real e = CUDDH_RK4_RATE(z, qs, c1, s1);
                        pa[l] -= third_dt * qs[l];
                        qa[l] += third * e;
                        ps[l] = p[l] - dt * qs[l];
                        qs[l] = q[l] + e;
                    }
                    sweep(ps, z);
#pragma unroll
                    for (int l = 0; l < N; ++l)
                    {
                        const Real e = CUDDH_RK4_RATE(z, qs, c2, s2);
                        p[l] = pa[l] - sixth_dt * qs[l];
                        q[l] = qa[l] + sixth * e;
                        u[l] += kw * p[l];
                        v[l] += kw * q[l];
                    }
                }
#undef CUDDH_RK4_RATE
            }
            else
            for (int it = 1; it <= nt; ++it)
            {
                const Real c0 = cs[2 * it - 2], s0 = sn[2 * it - 2];
                const Real c1 = cs[2 * it - 1], s1 = sn[2 * it - 1];
                const Real kw = filt[it];
                Real z[N], ph[N], qh[N];

                sweep(p, z);
#pragma unroll
                for (int l = 0; l < N; ++l)
                {
                    Real dq;
                    if constexpr (LEAN != 0)
                        dq = (((INTERIOR >> l) & 1u) ? (LEAN == 2 ? z[l] + c0 * F[l] + s0 * Gf[l] : z[l]) : (z[l] - Hi[l] * q[l]) + c0 * F[l] + s0 * Gf[l]);
                    else
                        dq = ((z[l] - Hi[l] * q[l]) + c0 * F[l] + s0 * Gf[l]) * invm[l];
                    ph[l] = p[l] - half_dt * q[l];
                    qh[l] = q[l] + (LEAN ? hm[l] : half_dt) * dq;
                    p[l] -= dt * qh[l];
                }
                sweep(ph, z);
#pragma unroll
                for (int l = 0; l < N; ++l)
                {
                    Real dq;
                    if constexpr (LEAN != 0)
                        dq = (((INTERIOR >> l) & 1u) ? (LEAN == 2 ? z[l] + c1 * F[l] + s1 * Gf[l] : z[l]) : (z[l] - Hi[l] * qh[l]) + c1 * F[l] + s1 * Gf[l]);
                    else
                        dq = ((z[l] - Hi[l] * qh[l]) + c1 * F[l] + s1 * Gf[l]) * invm[l];
                    q[l] += (LEAN ? dm[l] : dt) * dq;
                    u[l] += kw * p[l];
                    v[l] += kw * q[l];
                }
            }
        }
    }

    // Outputs of dof d of subdomain s from its filter sums u, v:  v /= omega,  y += M (u, v)  and, on the trace dofs, the
    // update -lambda -+ 2 a omega (v, u) through B.  unique_y: no other subdomain dof adds to these y entries (a vector layout
    // is set and the kernel honours it), so plain adds do; everything else adds atomically.
    template <typename Real>
    __device__ inline void publish_dof(const DdhArgs<Real> &A, int s, int d, int fdof, Real u, Real v, bool unique_y)
    {
        const size_t dbase = (size_t)A.mx_dof * s;
        v *= Real(1) / A.omega;
        if (A.y)
        {
            const int gidx = A.gI[dbase + d];
            const Real M = A.m[dbase + d] * A.gmi[dbase + d];
            if (unique_y)
            {
                A.y[gidx] += static_cast<double>(M * u);
                A.y[A.g_ndof + gidx] += static_cast<double>(M * v);
            }
            else
            {
                cuddh_k::atomic_add(A.y + gidx, static_cast<double>(M * u));
                cuddh_k::atomic_add(A.y + A.g_ndof + gidx, static_cast<double>(M * v));
            }
        }
        if (A.update && d < fdof)
        {
            const int wslot = A.B[d + (size_t)A.mx_fdof * (1 + 2 * (size_t)s)];
            if (wslot >= 0)
            {
                Real lam = 0, mu = 0;
                if (A.lambda)
                {
                    const int rslot = A.B[d + (size_t)A.mx_fdof * (0 + 2 * (size_t)s)];
                    if (rslot >= 0)
                    {
                        lam = A.lambda[rslot];
                        mu = A.lambda[A.n_lambda + rslot];
                    }
                }
                const Real S = Real(2) * A.a[dbase + d] * A.omega;
                A.update[wslot] = -lam - S * v;
                A.update[A.n_lambda + wslot] = -mu + S * u;
            }
        }
    }
} // namespace

#endif
