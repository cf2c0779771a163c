// DDH local solves (WaveHoltz time stepping of every subdomain) for gfx950.
//
// What is computed is the algorithm of reference source/DDH.cpp:111-321; how it
// is computed is different:
//   * the stiffness assembly is an owner gather in a fixed order, not float
//     atomics into LDS (source/DDH.cpp:108), so results are bitwise reproducible;
//   * `ddh_wave_kernel` (n_basis == 4, 4x4 elements) runs one subdomain per
//     WAVEFRONT with the whole state in registers: lane = (element, xi-node),
//     each lane owns the four eta-nodes of its column.  eta-direction
//     contractions are in-lane FMAs with scalar-register coefficients,
//     xi-direction contractions read the other three lanes of the quad through
//     DPP quad_perm operands, element-to-element assembly uses DPP row shifts
//     (xi neighbours) and one ds_bpermute pair (eta neighbours).  No LDS
//     storage, no barriers, 25,600 time steps per launch;
//   * `ddh_element_lane5_kernel` (n_basis == 5, 4x4 elements, rectangles) runs four
//     subdomains per wavefront, lane = element with its 25 nodes in registers:
//     both contractions in-lane, assembly by DPP row shifts inside a 16-lane row;
//   * `ddh_block_kernel` (any n_basis <= 10) runs one subdomain per workgroup
//     with the field staged in LDS, 3 barriers per stiffness sweep.
//
// Shape of the file: every local solve is  load_dof (per-dof coefficients)  ->
// wh_march (the WaveHoltz time stepping, RK2 or for an RK4 plan RK4, around a callable `sweep(w, z)`,
// z = S w)  ->  publish_dof (y and the trace update).  All six wavefront kernels
// use load_dof.  ddh_wave8_kernel, ddh_mfma_kernel<Real, ..> and
// ddh_element_lane_kernel (kernel 5's second sweep form: one element per lane,
// four subdomains per wavefront), ddh_element_lane8_kernel (kernel 11: the same
// with one 8x8-element subdomain per wavefront) and ddh_element_lane5_kernel
// (kernel 12: the 4x4 form at n_basis 5, 25 nodes per lane) use wh_march and publish_dof too and are a lane
// map, a sweep and an owner rule (which of the copies of a shared node
// publishes); the matrix-core and element-lane kernels take wh_march's LEAN
// forms, which leave out what their element-interior registers never need.
// ddh_wave_kernel keeps a copy of wh_march's
// loop and of publish_dof's body (on the shared ones it measured slower), and
// ddh_general_wave_kernel a copy of the loop (through a callable sweep it was
// not bitwise); see there.  ddh_block_kernel holds one value per
// thread and publishes the field to LDS before each sweep, with barriers inside
// it: its time loop has another shape and stays its own, and so do its load and
// publish, which keep a, m, gI and lambda in registers from one to the other
// (on the shared pair it re-reads them and compiles to different code); its
// CSR form (kernel 10) therefore has its own unique_y branch beside publish_dof's.
//
// Which kernel a plan runs is decided in ONE place, by host code without HIP (ddh_resolve.hpp: the kernel, the sweep form and
// the chain order in effect, from the shape, the request, the facts plan creation established and the options set since).
// resolve() calls it at the end of plan creation and of every setter whose argument enters it, and stores the outcome with
// the launch it means: a function that names the kernel's instantiation for the plan's state (n_basis, time grids, RK4,
// owner rule, chain order) and knows where its tables and trailing arguments come from.  apply() fills DdhArgs and calls that
// function; nothing is decided per launch but what belongs to the call (with or without x, priority).  Every kernel template
// is named in one hipLaunchKernelGGL (the run_* functions), runtime values become template arguments in with_flags and
// with_n_basis alone, and a combination that has no instantiation leaves the stored function null, which resolve() refuses:
// no launch of an RK4 plan can reach RK2 code.
#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "ddh_resolve.hpp"
#include "element_lane_tables.hpp"

using namespace cuddh_k;

struct cuddh_ddh_plan;

namespace
{
    template <typename Real>
    struct DdhArgs;

    // What resolve() stores for apply(): the function that launches the plan's kernel (the one for the plan's precision is set)
    // and the launch geometry, which depends on the plan alone.
    template <typename Real>
    using DdhRun = void (*)(const cuddh_ddh_plan *, const DdhArgs<Real> &, int n_local, hipStream_t);
    struct DdhLaunch
    {
        DdhRun<float> run32 = nullptr;
        DdhRun<double> run64 = nullptr;
        int per_group = 4;    // subdomains per workgroup: 4 (a wavefront each), 8 (kernels 6, 7), 16 (four per wavefront), 1 (kernels 1, 10)
        unsigned block = 256; // threads per workgroup (kernels 1 and 10: one per element node)
        size_t lds = 0;
    };
} // namespace

struct cuddh_ddh_plan
{
    cuddh_ddh_desc d;
    int is_f64;
    // what the plan runs, filled by resolve() and read by apply() and the queries.  now.kernel names the sweep:
    //  1 ddh_block_kernel (up to 1024 element nodes);  2 / 3 / 4 ddh_wave_kernel<Real, 0 / 1 / 2> (plain; hand-folded DPP FMAs, fp32;
    //  3 + MFMA for the in-lane contractions);  5 / 8 ddh_mfma_kernel<float / double> (dense element matrix on the matrix
    //  cores, uniform geometry; 5 in sweep form now.form, 2 and 3: ddh_element_lane_kernel in chain order now.order);
    //  6 / 7 ddh_wave8_kernel (nb == 8; 7 separable, fp32);  9 ddh_general_wave_kernel
    //  (nb == 4, <= 16 elements, CSR lists);  10 ddh_block_kernel with CSR lists;  11 ddh_element_lane8_kernel (nb == 4,
    //  8x8 elements, fp32: one element per lane, one subdomain per wavefront);  12 ddh_element_lane5_kernel (nb == 5, 4x4
    //  elements, fp32: one element per lane, four subdomains per wavefront);  13 on request: the element-lane kernels
    //  with four subdomains per wavefront (nb == 4 or 5, 4x4 elements, fp32) that take per-subdomain time grids
    DdhResolved now{0, 0, 0};
    DdhLaunch launch;
    unsigned facts = 0; // what plan creation established about the descriptor (ddh_fact bits, establish_facts)
    int mx_elems = 0;   // general plans: elements per subdomain at most; 0: a structured plan
    int nodes;  // nb*nb*nel1d*nel1d (general plans: nb*nb*mx_elems)
    int wh_iters = 5; // WaveHoltz iterations per local solve (source/DDH.cpp:136); WH_ITERS_REFERENCE
    const int *gI_override = nullptr; // cuddh_hip_ddh_plan_set_vector_layout: x and y in another numbering than d.gI
    int g_ndof_override = 0;
    float *Aop = nullptr; // kernel 5: element stiffness matrix as MFMA A operands, [4 k-steps][64 lanes]
    double *Aop64 = nullptr; // kernel 8: the same in fp64, rows in the f64 MFMA's output order (build_dense_element_matrix)
    float *Sep = nullptr; // kernel 7: [Ax | Ay | beta | gamma] of the separable nb = 8 sweep
    float *Sep4 = nullptr; // kernel 5, element-lane form, and kernel 11: [Bx | By | Dg | W | 1 / W] (build_element_lane_tables); null: does not qualify.
                           // kernel 12: the same table with 5 in place of 4
    int last_copy = 0; // kernels 11, 12 and 13: the last copy of a shared node publishes, not the first (cuddh_hip_ddh_plan_set_owner_rule)
    int sweep_form = 0; // kernel 5: 0 auto, 1 matrix form, 2 element-lane form, 3 the same with the other owner rule (cuddh_hip_ddh_plan_set_sweep_form)
    int chain_order = 0; // kernel 5's element-lane form: 0 auto, 1 pinned chains, 2 paired chains (cuddh_hip_ddh_plan_set_chain_order)
    int wave_priority = 0; // cuddh_hip_ddh_plan_set_wave_priority
    // general plans (cuddh_hip_ddh_plan_create_general; kernels 9 and 10): assembly lists, see DdhArgs::csr_off
    int *csr_off = nullptr, *csr_src = nullptr;
    int requested = 0; // the kernel the caller asked for (0 auto): cuddh_hip_ddh_plan_set_time_grids moves an auto choice, never a request
    // per-subdomain time grids (cuddh_hip_ddh_plan_set_time_grids).  n_grids == 0: every subdomain marches on the descriptor's grid
    int n_grids = 0;
    void *grids = nullptr;          // DdhTimeGrid<Real>[n_grids], DEVICE, the plan's
    const int *grid_of = nullptr;   // (n_domains) DEVICE, the caller's, like the three concatenated tables
    const void *grid_filter = nullptr, *grid_cs = nullptr, *grid_sn = nullptr;
    int *by_steps = nullptr;        // (n_domains) DEVICE: the subdomains by step count descending, stable by index; what a full-range apply lists
    int *by_index = nullptr;        // (n_domains) DEVICE: 0, 1, 2, ...; what an apply over a sub-range lists
    int rk4 = 0; // cuddh_hip_ddh_plan_set_integrator: the local solves step with classical RK4 (four sweeps per step), not RK2
};

namespace
{
    constexpr int WH_ITERS_REFERENCE = 5; // WaveHoltz iterations of the reference (source/DDH.cpp:136)

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
    // ddh_element_lane_kernel and ddh_element_lane5_kernel hold a subdomain per 16-lane DPP row and one time grid per march.
    // Their TimeGrids instantiations march once per distinct grid among the wavefront's rows: a pass takes the lowest row
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

    // Issue priority of the calling wavefront (s_setprio).  All wavefronts of one rank's local solves are resident at once and
    // advance at the same rate, so a launch of the few subdomains whose traces other ranks wait for finishes no earlier than
    // the launch of all the others it shares the SIMDs with (profiles/r02/overlap_timeline.txt) -- unless its wavefronts are
    // issued first whenever they are ready.
    __device__ inline void raise_priority(int prio)
    {
        if (prio)
            __builtin_amdgcn_s_setprio(3);
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
                atomic_add(A.y + gidx, static_cast<double>(M * u));
                atomic_add(A.y + A.g_ndof + gidx, static_cast<double>(M * v));
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

    // ---------------------------------------------------------------- DPP helpers
    template <int CTRL>
    __device__ inline float dpp_read(float v)
    {
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
    }

    template <int CTRL>
    __device__ inline double dpp_read(double v)
    {
        const long long bits = __double_as_longlong(v);
        const int lo = __builtin_amdgcn_update_dpp(0, static_cast<int>(bits), CTRL, 0xf, 0xf, true);
        const int hi = __builtin_amdgcn_update_dpp(0, static_cast<int>(bits >> 32), CTRL, 0xf, 0xf, true);
        return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned int>(lo));
    }

    constexpr int QUAD_BCAST(int i) { return i * 0x55; } // quad_perm:[i,i,i,i]
    constexpr int ROW_SHL1 = 0x101;                      // lane j reads lane j+1 of its 16-lane row
    constexpr int ROW_SHR1 = 0x111;                      // lane j reads lane j-1

    // ---------------------------------------------------------------- wavefront-per-subdomain kernel (NB = 4, 4x4 elements)

    // out[l] = sum_i c[i] * (value of in[l] in lane i of my quad), l = 0..3.
    // Generic form: the compiler emits v_mov_b32_dpp + FMA pairs.
    template <typename Real>
    __device__ inline void quad_contract(const Real (&in)[4], const Real (&c)[4], Real (&out)[4])
    {
#pragma unroll
        for (int l = 0; l < 4; ++l)
        {
            Real s = c[0] * dpp_read<QUAD_BCAST(0)>(in[l]);
            s += c[1] * dpp_read<QUAD_BCAST(1)>(in[l]);
            s += c[2] * dpp_read<QUAD_BCAST(2)>(in[l]);
            s += c[3] * dpp_read<QUAD_BCAST(3)>(in[l]);
            out[l] = s;
        }
    }

    // fp32 form with the cross-lane read folded into the FMA (v_fmac_f32_dpp): 16 VALU instructions
    // instead of 32.  hipcc does not fold a DPP move into an accumulating FMA by itself.  The leading
    // s_nop covers the "VALU write -> DPP read" hazard (2 wait states) for the inputs; inside the block
    // DPP operands are only the (unmodified) inputs.
#define CUDDH_QP(i) " quad_perm:[" #i "," #i "," #i "," #i "] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
    __device__ inline void quad_contract_asm(const float (&in)[4], const float (&c)[4], float (&out)[4])
    {
        float o0, o1, o2, o3;
        asm volatile("s_nop 1\n\t"
                     "v_mul_f32_dpp %0, %4, %8" CUDDH_QP(0)
                     "v_mul_f32_dpp %1, %5, %8" CUDDH_QP(0)
                     "v_mul_f32_dpp %2, %6, %8" CUDDH_QP(0)
                     "v_mul_f32_dpp %3, %7, %8" CUDDH_QP(0)
                     "v_fmac_f32_dpp %0, %4, %9" CUDDH_QP(1)
                     "v_fmac_f32_dpp %1, %5, %9" CUDDH_QP(1)
                     "v_fmac_f32_dpp %2, %6, %9" CUDDH_QP(1)
                     "v_fmac_f32_dpp %3, %7, %9" CUDDH_QP(1)
                     "v_fmac_f32_dpp %0, %4, %10" CUDDH_QP(2)
                     "v_fmac_f32_dpp %1, %5, %10" CUDDH_QP(2)
                     "v_fmac_f32_dpp %2, %6, %10" CUDDH_QP(2)
                     "v_fmac_f32_dpp %3, %7, %10" CUDDH_QP(2)
                     "v_fmac_f32_dpp %0, %4, %11" CUDDH_QP(3)
                     "v_fmac_f32_dpp %1, %5, %11" CUDDH_QP(3)
                     "v_fmac_f32_dpp %2, %6, %11" CUDDH_QP(3)
                     "v_fmac_f32_dpp %3, %7, %11" CUDDH_QP(3)
                     : "=&v"(o0), "=&v"(o1), "=&v"(o2), "=&v"(o3)
                     : "v"(in[0]), "v"(in[1]), "v"(in[2]), "v"(in[3]), "v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(c[3]));
        out[0] = o0;
        out[1] = o1;
        out[2] = o2;
        out[3] = o3;
    }

    // r[l] = mR * (z[l] of lane+1) + mL * (z[l] of lane-1) within the 16-lane row, fp32, 8 instructions
    __device__ inline void row_neighbours_asm(const float (&z)[4], float mR, float mL, float (&r)[4])
    {
        float o0, o1, o2, o3;
        asm volatile("s_nop 1\n\t"
                     "v_mul_f32_dpp %0, %4, %8 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_mul_f32_dpp %1, %5, %8 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_mul_f32_dpp %2, %6, %8 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_mul_f32_dpp %3, %7, %8 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %0, %4, %9 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %1, %5, %9 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %2, %6, %9 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %3, %7, %9 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     : "=&v"(o0), "=&v"(o1), "=&v"(o2), "=&v"(o3)
                     : "v"(z[0]), "v"(z[1]), "v"(z[2]), "v"(z[3]), "v"(mR), "v"(mL));
        r[0] = o0;
        r[1] = o1;
        r[2] = o2;
        r[3] = o3;
    }
#undef CUDDH_QP

    // VAR 0: plain HIP; 1: DPP reads folded into the FMAs (fp32); 2: as 1, and the in-lane (eta) contractions run on the
    // matrix pipe as v_mfma_f32_4x4x1_16b_f32 (one 4x4 block per element, exact fp32 FMA chains), beside the VALU
    // Element-local part of one stiffness sweep: zz[l] = (S_el w)(k, l) for the element of my quad (no assembly).
    template <int VAR, typename Real>
    __device__ inline void wave_element_stiffness(const Real (&w)[4], Real (&zz)[4], const Real (&gx)[4], const Real (&gy)[4],
                                                  const Real (&gz)[4], const Real (&Dk)[4], const Real (&DTk)[4], const Real *__restrict__ Dm)
    {
        constexpr bool ASM = VAR >= 1;
        Real ux[4], uy[4];
        // eta derivative uy(k,l) = sum_i D(l,i) u(k,i): in-lane
        if constexpr (VAR == 2)
        {
            // block = element, output row = l (register), column = k (lane): A_b[l] = D(l,i) is lane k==l's Dk[i],
            // B_b[k] = u(k,i) is my w[i]
            typedef float f4 __attribute__((ext_vector_type(4)));
            f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int i = 0; i < 4; ++i)
                acc = __builtin_amdgcn_mfma_f32_4x4x1f32(Dk[i], w[i], acc, 0, 0, 0);
#pragma unroll
            for (int l = 0; l < 4; ++l)
                uy[l] = acc[l];
        }
        else
        {
#pragma unroll
            for (int l = 0; l < 4; ++l)
            {
                Real s = Dm[l] * w[0];
#pragma unroll
                for (int i = 1; i < 4; ++i)
                    s += Dm[l + 4 * i] * w[i];
                uy[l] = s;
            }
        }
        // xi derivative: u(i, l) sits in lane i of my quad
        if constexpr (ASM)
            quad_contract_asm(w, Dk, ux);
        else
            quad_contract(w, Dk, ux);
        Real f1[4], f2[4];
#pragma unroll
        for (int l = 0; l < 4; ++l)
        {
            f1[l] = gx[l] * ux[l] + gy[l] * uy[l];
            f2[l] = gy[l] * ux[l] + gz[l] * uy[l];
        }
        // test functions: sum_i D(i,k) f1(i,l)  +  sum_i D(i,l) f2(k,i)
        if constexpr (ASM)
            quad_contract_asm(f1, DTk, zz);
        else
            quad_contract(f1, DTk, zz);
        if constexpr (VAR == 2)
        {
            // A_b[l] = D(i,l) is lane k==l's DTk[i], B_b[k] = f2(k,i) is my f2[i]; accumulate onto the xi part
            typedef float f4 __attribute__((ext_vector_type(4)));
            f4 acc = {zz[0], zz[1], zz[2], zz[3]};
#pragma unroll
            for (int i = 0; i < 4; ++i)
                acc = __builtin_amdgcn_mfma_f32_4x4x1f32(DTk[i], f2[i], acc, 0, 0, 0);
#pragma unroll
            for (int l = 0; l < 4; ++l)
                zz[l] = acc[l];
        }
        else
        {
#pragma unroll
            for (int l = 0; l < 4; ++l)
            {
                Real s = zz[l];
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    s += Dm[i + 4 * l] * f2[i];
                zz[l] = s;
            }
        }
    }

    template <int VAR, typename Real>
    __device__ inline void wave_stiffness(const Real (&w)[4], Real (&z)[4], const Real (&gx)[4], const Real (&gy)[4], const Real (&gz)[4],
                                          const Real (&Dk)[4], const Real (&DTk)[4], const Real *__restrict__ Dm, Real mR, Real mL,
                                          Real mU, Real mD, int lane)
    {
        constexpr bool ASM = VAR >= 1;
        Real zz[4];
        wave_element_stiffness<VAR>(w, zz, gx, gy, gz, Dk, DTk, Dm);
        // assembly across elements.  xi neighbours: my k==3 column meets the k==0 column of lane+1 (and vice versa)
        if constexpr (ASM)
        {
            Real r[4];
            row_neighbours_asm(zz, mR, mL, r);
#pragma unroll
            for (int l = 0; l < 4; ++l)
                z[l] = zz[l] + r[l];
        }
        else
        {
#pragma unroll
            for (int l = 0; l < 4; ++l)
            {
                const Real from_right = dpp_read<ROW_SHL1>(zz[l]);
                const Real from_left = dpp_read<ROW_SHR1>(zz[l]);
                z[l] = zz[l] + (mR * from_right + mL * from_left);
            }
        }
        // eta neighbours: my l==3 node meets the l==0 node of lane+16 (and vice versa)
        {
            const Real top = z[3], bottom = z[0];
            const Real from_above = __shfl(bottom, (lane + 16) & 63, 64);
            const Real from_below = __shfl(top, (lane + 48) & 63, 64);
            z[3] = top + mU * from_above;
            z[0] = bottom + mD * from_below;
        }
    }

    template <typename Real, int VAR, typename... Grids>
    __global__ void __launch_bounds__(256) ddh_wave_kernel(DdhArgs<Real> A, const Real *__restrict__ Dmat, const Real *__restrict__ filt,
                                                          const Real *__restrict__ cs, const Real *__restrict__ sn, Grids... grids)
    {
        const int lane = threadIdx.x & 63;
        const int position = A.dom_begin + blockIdx.x * 4 + (threadIdx.x >> 6);
        if (position >= A.dom_end)
            return; // wave-uniform: the kernel has no barriers
        const int s = domain_at(A, position, grids...);
        raise_priority(A.prio);

        const int k = lane & 3, el = lane >> 2, ex = el & 3, ey = el >> 2;
        const int fdof = A.s_fdof[s];
        const int *sI = A.sI + 256 * (size_t)s;
        const size_t dbase = (size_t)A.mx_dof * s;

        Real gx[4], gy[4], gz[4], invm[4], Hi[4], F[4], Gf[4], u[4], v[4];
#pragma unroll
        for (int l = 0; l < 4; ++l)
        {
            const int node = k + 4 * (l + 4 * el);
            const int d = sI[node];
            const Real *g = A.G + 3 * ((size_t)node + 256 * (size_t)s);
            gx[l] = g[0];
            gy[l] = g[1];
            gz[l] = g[2];
            load_dof(A, s, d, fdof, invm[l], Hi[l], F[l], Gf[l]);
        }

        Real Dk[4], DTk[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
        {
            Dk[i] = Dmat[k + 4 * i];  // D(k, i)
            DTk[i] = Dmat[i + 4 * k]; // D(i, k)
        }
        const Real mR = (k == 3 && ex < 3) ? Real(1) : Real(0);
        const Real mL = (k == 0 && ex > 0) ? Real(1) : Real(0);
        const Real mU = (ey < 3) ? Real(1) : Real(0);
        const Real mD = (ey > 0) ? Real(1) : Real(0);

        // A copy of wh_march's loop, and below it of publish_dof's body.  On wh_march (sweep as a callable) the results stay
        // bitwise but the compiler schedules the time loop differently, and the folded-DPP form (kernel 3, what auto picks on
        // non-uniform geometry) measured 0.6 % slower than before in five of five alternating rounds, against 0.2 % spread;
        // with the loop written out and publish_dof, the loop's instructions are the previous ones but the registers are not,
        // and kernel 4 measured 0.5 % slower in three of three rounds against 0.1 % (profiles/r06/ddh_rates_ab.txt).  As it
        // stands all four instantiations compile to the previous assembly text, registers included.  Any change to wh_march
        // or publish_dof is made here as well (and, for wh_march, in ddh_general_wave_kernel).
        // The RK4 form has no earlier commit to stay bitwise equal to: it is wh_march with the sweep as a callable.
        Real p[4], q[4];
#pragma unroll
        for (int l = 0; l < 4; ++l)
            p[l] = q[l] = u[l] = v[l] = 0;
        const TimeGridView<Real> tg = time_grid_of(A, s, filt, cs, sn, grids...);
        if constexpr (scheme_of<Grids...> == 1)
        {
            wh_march<0, 1u, 1>(A, tg.nt, tg.dt, tg.filt, tg.cs, tg.sn, invm, Hi, F, Gf, u, v, [&](const Real(&w)[4], Real(&z)[4])
                               { wave_stiffness<VAR>(w, z, gx, gy, gz, Dk, DTk, Dmat, mR, mL, mU, mD, lane); });
        }
        else
        {
        const Real dt = tg.dt, half_dt = Real(0.5) * tg.dt;
        const int nt = tg.nt;

        for (int whit = 0; whit < A.wh_iters; ++whit)
        {
            {
                const Real k0 = tg.filt[0];
#pragma unroll
                for (int l = 0; l < 4; ++l)
                {
                    p[l] = u[l];
                    q[l] = v[l];
                    u[l] *= k0;
                    v[l] *= k0;
                }
            }
            for (int it = 1; it <= nt; ++it)
            {
                const Real c0 = tg.cs[2 * it - 2], s0 = tg.sn[2 * it - 2];
                const Real c1 = tg.cs[2 * it - 1], s1 = tg.sn[2 * it - 1];
                const Real kw = tg.filt[it];
                Real z[4], ph[4], qh[4];

                wave_stiffness<VAR>(p, z, gx, gy, gz, Dk, DTk, Dmat, mR, mL, mU, mD, lane);
#pragma unroll
                for (int l = 0; l < 4; ++l)
                {
                    const Real dq = ((z[l] - Hi[l] * q[l]) + c0 * F[l] + s0 * Gf[l]) * invm[l];
                    ph[l] = p[l] - half_dt * q[l];
                    qh[l] = q[l] + half_dt * dq;
                    p[l] -= dt * qh[l];
                }
                wave_stiffness<VAR>(ph, z, gx, gy, gz, Dk, DTk, Dmat, mR, mL, mU, mD, lane);
#pragma unroll
                for (int l = 0; l < 4; ++l)
                {
                    const Real dq = ((z[l] - Hi[l] * qh[l]) + c1 * F[l] + s1 * Gf[l]) * invm[l];
                    q[l] += dt * dq;
                    u[l] += kw * p[l];
                    v[l] += kw * q[l];
                }
            }
        }
        }

        const Real rw = Real(1) / A.omega;
#pragma unroll
        for (int l = 0; l < 4; ++l)
        {
            v[l] *= rw;
            // every shared node is held by 2 or 4 (lane, l) pairs with identical values: the copy with
            // the smallest element-node index writes
            const bool owner = !(k == 0 && ex > 0) && !(l == 0 && ey > 0);
            if (!owner)
                continue;
            const int d = sI[k + 4 * (l + 4 * el)];
            if (A.y)
            {
                const int gidx = A.gI[dbase + d];
                const Real M = A.m[dbase + d] * A.gmi[dbase + d];
                atomic_add(A.y + gidx, static_cast<double>(M * u[l]));
                atomic_add(A.y + A.g_ndof + gidx, static_cast<double>(M * v[l]));
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
                    A.update[wslot] = -lam - S * v[l];
                    A.update[A.n_lambda + wslot] = -mu + S * u[l];
                }
            }
        }
    }

    // ---------------------------------------------------------------- kernel 9: wavefront per unstructured subdomain (NB = 4)
    // Element-local part as kernel 3: lane = (element, xi-node) of up to 16 elements, the four eta-nodes of the lane's column
    // in registers, DPP quad contractions.  The RK2 state stays per element node (copies of a shared dof hold bitwise equal
    // values: every copy reads the same assembled sum and the same per-dof coefficients).  Assembly goes through wave-private
    // LDS: every lane writes its four element contributions, then lane j forms the sums of dofs j, j + 64, j + 128, j + 192
    // along the plan's CSR lists (ascending element node, any valence), then every node reads its dof's sum back through sI.
    // A wavefront owns its subdomain, so the LDS phases are ordered by wave-level fences only (DS instructions of one
    // wavefront execute in order; the fence keeps the compiler from moving them and makes it wait for the data).
    constexpr int GW_NODES = 256; // element nodes (and dofs) per subdomain at most

    __device__ inline void wave_lds_fence()
    {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }

    // LDS slot of element node (k, l, el): lane-major, so a lane's four contributions are contiguous
    __device__ inline int gw_slot(int node) { return ((node >> 4) << 4) + ((node & 3) << 2) + ((node >> 2) & 3); }

    template <typename Real>
    __device__ inline void gw_assemble(const Real (&zz)[4], Real (&z)[4], Real *__restrict__ s_c, Real *__restrict__ s_d,
                                       const int *__restrict__ s_src, const int (&st)[4], const int (&ct)[4], const int (&dof)[4], int lane)
    {
#pragma unroll
        for (int l = 0; l < 4; ++l)
            s_c[4 * lane + l] = zz[l];
        wave_lds_fence();
#pragma unroll
        for (int j = 0; j < 4; ++j)
        {
            Real sum = 0;
            for (int c = 0; c < ct[j]; ++c)
                sum += s_c[s_src[st[j] + c]];
            s_d[lane + 64 * j] = sum;
        }
        wave_lds_fence();
#pragma unroll
        for (int l = 0; l < 4; ++l)
            z[l] = s_d[dof[l]];
    }

    template <typename Real, int VAR, typename... Grids>
    __global__ void __launch_bounds__(256) ddh_general_wave_kernel(DdhArgs<Real> A, const Real *__restrict__ Dmat, const Real *__restrict__ filt,
                                                                  const Real *__restrict__ cs, const Real *__restrict__ sn, Grids... grids)
    {
        __shared__ Real lds_c[4][GW_NODES], lds_d[4][GW_NODES];
        __shared__ int lds_src[4][GW_NODES];
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int position = A.dom_begin + blockIdx.x * 4 + wave;
        if (position >= A.dom_end)
            return; // wave-uniform: the kernel has no workgroup barriers
        const int s = domain_at(A, position, grids...);
        raise_priority(A.prio);
        Real *s_c = lds_c[wave], *s_d = lds_d[wave];
        int *s_src = lds_src[wave];

        const int T = A.nodes; // 16 * mx_elems <= 256: stride of sI, G and the CSR lists
        const int k = lane & 3, el = lane >> 2;
        const int ndof = A.s_dof[s], fdof = A.s_fdof[s];
        const int *sI = A.sI + (size_t)T * s;
        const int *off = A.csr_off + (size_t)(T + 1) * s;
        const int *src = A.csr_src + (size_t)T * s;

        // CSR lists: sources as LDS slots in LDS, (start, count) of my four dofs in registers
        int st[4], ct[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
        {
            const int d = lane + 64 * j;
            st[j] = ct[j] = 0;
            if (d < ndof)
            {
                st[j] = off[d];
                ct[j] = off[d + 1] - st[j];
            }
            if (d < T)
                s_src[d] = d < off[ndof] ? gw_slot(src[d]) : 0;
        }

        Real gx[4], gy[4], gz[4], invm[4], Hi[4], F[4], Gf[4];
        Real p[4], q[4], u[4], v[4];
        int dof[4];
#pragma unroll
        for (int l = 0; l < 4; ++l)
        {
            const int node = k + 4 * (l + 4 * el);
            const int d = node < T ? sI[node] : -1; // -1: no element here (padding of a smaller subdomain)
            dof[l] = d < 0 ? 0 : d;
            gx[l] = gy[l] = gz[l] = invm[l] = Hi[l] = F[l] = Gf[l] = 0;
            p[l] = q[l] = u[l] = v[l] = 0;
            if (d < 0)
                continue;
            const Real *g = A.G + 3 * ((size_t)node + (size_t)T * s);
            gx[l] = g[0];
            gy[l] = g[1];
            gz[l] = g[2];
            load_dof(A, s, d, fdof, invm[l], Hi[l], F[l], Gf[l]);
        }

        Real Dk[4], DTk[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
        {
            Dk[i] = Dmat[k + 4 * i];  // D(k, i)
            DTk[i] = Dmat[i + 4 * k]; // D(i, k)
        }
        wave_lds_fence(); // s_src complete before the first assembly reads it

        // A second copy of wh_march's loop.  With this kernel's sweep as a callable, -ffp-contract=fast fuses the other of the
        // two products of gx ux + gy uy in wave_element_stiffness and the results move in the last bits (on the GPU against the
        // commit before: 16 of 225 output arrays, all kernel 9's; with this copy 225 of 225 are bitwise equal,
        // profiles/r06/ddh_bitwise_vs_parent.txt).  Writing the FMA out in wave_element_stiffness does not settle it: the form
        // the compiler picks here is not the one it picks for ddh_wave_kernel, so one explicit form moves one of the two.
        // Any change to wh_march is made here and in ddh_wave_kernel as well.
        // The RK4 form has no earlier commit to stay bitwise equal to: it is wh_march with the sweep as a callable.  The
        // wavefronts of a workgroup may run different step counts (time grids): the LDS is wave-private and nothing here
        // is a workgroup barrier.
        const TimeGridView<Real> tg = time_grid_of(A, s, filt, cs, sn, grids...);
        if constexpr (scheme_of<Grids...> == 1)
        {
            wh_march<0, 1u, 1>(A, tg.nt, tg.dt, tg.filt, tg.cs, tg.sn, invm, Hi, F, Gf, u, v, [&](const Real(&w)[4], Real(&z)[4])
                               {
                                   Real zz[4];
                                   wave_element_stiffness<VAR>(w, zz, gx, gy, gz, Dk, DTk, Dmat);
                                   gw_assemble(zz, z, s_c, s_d, s_src, st, ct, dof, lane);
                               });
        }
        else
        {
        const Real dt = tg.dt, half_dt = Real(0.5) * tg.dt;
        const int nt = tg.nt;

        for (int whit = 0; whit < A.wh_iters; ++whit)
        {
            {
                const Real k0 = tg.filt[0];
#pragma unroll
                for (int l = 0; l < 4; ++l)
                {
                    p[l] = u[l];
                    q[l] = v[l];
                    u[l] *= k0;
                    v[l] *= k0;
                }
            }
            for (int it = 1; it <= nt; ++it)
            {
                const Real c0 = tg.cs[2 * it - 2], s0 = tg.sn[2 * it - 2];
                const Real c1 = tg.cs[2 * it - 1], s1 = tg.sn[2 * it - 1];
                const Real kw = tg.filt[it];
                Real zz[4], z[4], ph[4], qh[4];

                wave_element_stiffness<VAR>(p, zz, gx, gy, gz, Dk, DTk, Dmat);
                gw_assemble(zz, z, s_c, s_d, s_src, st, ct, dof, lane);
#pragma unroll
                for (int l = 0; l < 4; ++l)
                {
                    const Real dq = ((z[l] - Hi[l] * q[l]) + c0 * F[l] + s0 * Gf[l]) * invm[l];
                    ph[l] = p[l] - half_dt * q[l];
                    qh[l] = q[l] + half_dt * dq;
                    p[l] -= dt * qh[l];
                }
                wave_element_stiffness<VAR>(ph, zz, gx, gy, gz, Dk, DTk, Dmat);
                gw_assemble(zz, z, s_c, s_d, s_src, st, ct, dof, lane);
#pragma unroll
                for (int l = 0; l < 4; ++l)
                {
                    const Real dq = ((z[l] - Hi[l] * qh[l]) + c1 * F[l] + s1 * Gf[l]) * invm[l];
                    q[l] += dt * dq;
                    u[l] += kw * p[l];
                    v[l] += kw * q[l];
                }
            }
        }
        }

        // outputs per dof: the copy at the dof's first contributing element node publishes u, v
#pragma unroll
        for (int l = 0; l < 4; ++l)
        {
            s_c[4 * lane + l] = u[l];
            s_d[4 * lane + l] = v[l];
        }
        wave_lds_fence();
#pragma unroll
        for (int j = 0; j < 4; ++j)
        {
            const int d = lane + 64 * j;
            if (d >= ndof)
                continue;
            const int first = s_src[st[j]];
            publish_dof(A, s, d, fdof, s_c[first], s_d[first], A.unique_y != 0);
        }
    }

    // ---------------------------------------------------------------- wavefront per TWO subdomains (NB = 8, 2x2 elements)
    // The reference's other supported shape (source/DDH.cpp:631-636).  lane = k + 8 * element + 32 * (subdomain of the
    // pair); every lane owns the eight eta-nodes of its column, so eta contractions are 8x8 in-lane FMAs with scalar
    // coefficients.  The xi contraction runs over the eight lanes of an octet: partner k^x for x = 1,2,3 is a DPP
    // quad_perm operand, k^7 is row_half_mirror, and k^4, k^5, k^6 are quad_perms of the half-mirrored copy; the
    // coefficient of partner x is the per-lane register D(k, k^x).  xi neighbours (ex 0|1) sit in adjacent lanes 7|8 of a
    // 16-lane row (DPP row shifts), eta neighbours (ey 0|1) 16 lanes apart (one ds_bpermute pair per sweep).
    constexpr int QP_XOR1 = 0xB1, QP_XOR2 = 0x4E, QP_XOR3 = 0x1B, ROW_HALF_MIRROR = 0x141;

    // out[l] = sum_x c[x] * (in[l] of lane k^x of my octet)
    template <typename Real>
    __device__ inline void octet_contract(const Real (&in)[8], const Real (&c)[8], Real (&out)[8])
    {
#pragma unroll
        for (int l = 0; l < 8; ++l)
        {
            const Real t = dpp_read<ROW_HALF_MIRROR>(in[l]);
            Real s = c[0] * in[l];
            s += c[1] * dpp_read<QP_XOR1>(in[l]);
            s += c[2] * dpp_read<QP_XOR2>(in[l]);
            s += c[3] * dpp_read<QP_XOR3>(in[l]);
            s += c[7] * t;
            s += c[6] * dpp_read<QP_XOR1>(t);
            s += c[5] * dpp_read<QP_XOR2>(t);
            s += c[4] * dpp_read<QP_XOR3>(t);
            out[l] = s;
        }
    }

    // fp32 form with the cross-lane reads folded into the FMAs: 36 VALU instructions per four nodes.  The half-mirrored
    // copies are written first and read through DPP at least four instructions later (the hazard needs two).
#define CUDDH_DPP_TAIL " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
#define CUDDH_X1 " quad_perm:[1,0,3,2]" CUDDH_DPP_TAIL
#define CUDDH_X2 " quad_perm:[2,3,0,1]" CUDDH_DPP_TAIL
#define CUDDH_X3 " quad_perm:[3,2,1,0]" CUDDH_DPP_TAIL
    __device__ inline void octet_contract4_asm(const float *in, const float (&c)[8], float *out)
    {
        float o0, o1, o2, o3, t0, t1, t2, t3;
        asm volatile("s_nop 1\n\t"
                     "v_mov_b32_dpp %4, %8 row_half_mirror" CUDDH_DPP_TAIL
                     "v_mov_b32_dpp %5, %9 row_half_mirror" CUDDH_DPP_TAIL
                     "v_mov_b32_dpp %6, %10 row_half_mirror" CUDDH_DPP_TAIL
                     "v_mov_b32_dpp %7, %11 row_half_mirror" CUDDH_DPP_TAIL
                     "v_mul_f32 %0, %8, %12\n\t"
                     "v_mul_f32 %1, %9, %12\n\t"
                     "v_mul_f32 %2, %10, %12\n\t"
                     "v_mul_f32 %3, %11, %12\n\t"
                     "v_fmac_f32_dpp %0, %8, %13" CUDDH_X1
                     "v_fmac_f32_dpp %1, %9, %13" CUDDH_X1
                     "v_fmac_f32_dpp %2, %10, %13" CUDDH_X1
                     "v_fmac_f32_dpp %3, %11, %13" CUDDH_X1
                     "v_fmac_f32_dpp %0, %8, %14" CUDDH_X2
                     "v_fmac_f32_dpp %1, %9, %14" CUDDH_X2
                     "v_fmac_f32_dpp %2, %10, %14" CUDDH_X2
                     "v_fmac_f32_dpp %3, %11, %14" CUDDH_X2
                     "v_fmac_f32_dpp %0, %8, %15" CUDDH_X3
                     "v_fmac_f32_dpp %1, %9, %15" CUDDH_X3
                     "v_fmac_f32_dpp %2, %10, %15" CUDDH_X3
                     "v_fmac_f32_dpp %3, %11, %15" CUDDH_X3
                     "v_fmac_f32 %0, %4, %19\n\t"
                     "v_fmac_f32 %1, %5, %19\n\t"
                     "v_fmac_f32 %2, %6, %19\n\t"
                     "v_fmac_f32 %3, %7, %19\n\t"
                     "v_fmac_f32_dpp %0, %4, %18" CUDDH_X1
                     "v_fmac_f32_dpp %1, %5, %18" CUDDH_X1
                     "v_fmac_f32_dpp %2, %6, %18" CUDDH_X1
                     "v_fmac_f32_dpp %3, %7, %18" CUDDH_X1
                     "v_fmac_f32_dpp %0, %4, %17" CUDDH_X2
                     "v_fmac_f32_dpp %1, %5, %17" CUDDH_X2
                     "v_fmac_f32_dpp %2, %6, %17" CUDDH_X2
                     "v_fmac_f32_dpp %3, %7, %17" CUDDH_X2
                     "v_fmac_f32_dpp %0, %4, %16" CUDDH_X3
                     "v_fmac_f32_dpp %1, %5, %16" CUDDH_X3
                     "v_fmac_f32_dpp %2, %6, %16" CUDDH_X3
                     "v_fmac_f32_dpp %3, %7, %16" CUDDH_X3
                     : "=&v"(o0), "=&v"(o1), "=&v"(o2), "=&v"(o3), "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3)
                     : "v"(in[0]), "v"(in[1]), "v"(in[2]), "v"(in[3]), "v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(c[3]), "v"(c[4]), "v"(c[5]),
                       "v"(c[6]), "v"(c[7]));
        out[0] = o0;
        out[1] = o1;
        out[2] = o2;
        out[3] = o3;
    }
#undef CUDDH_X1
#undef CUDDH_X2
#undef CUDDH_X3
#undef CUDDH_DPP_TAIL

    template <bool ASM, typename Real>
    __device__ inline void octet_contract_any(const Real (&in)[8], const Real (&c)[8], Real (&out)[8])
    {
        if constexpr (ASM && sizeof(Real) == 4)
        {
            octet_contract4_asm(&in[0], c, &out[0]);
            octet_contract4_asm(&in[4], c, &out[4]);
        }
        else
            octet_contract(in, c, out);
    }

    template <bool ASM, typename Real>
    __device__ inline void wave8_stiffness(const Real (&w)[8], Real (&z)[8], const Real (&gx)[8], const Real (&gy)[8], const Real (&gz)[8],
                                           const Real (&Dk)[8], const Real (&DTk)[8], const Real *__restrict__ Dm, Real mR, Real mL,
                                           Real mU, Real mD, int lane)
    {
        Real ux[8], uy[8];
        // eta derivative uy(k,l) = sum_i D(l,i) u(k,i): in-lane, scalar coefficients
#pragma unroll
        for (int l = 0; l < 8; ++l)
        {
            Real s = Dm[l] * w[0];
#pragma unroll
            for (int i = 1; i < 8; ++i)
                s += Dm[l + 8 * i] * w[i];
            uy[l] = s;
        }
        // xi derivative ux(k,l) = sum_i D(k,i) u(i,l): over the octet
        octet_contract_any<ASM>(w, Dk, ux);
        Real f1[8], f2[8];
#pragma unroll
        for (int l = 0; l < 8; ++l)
        {
            f1[l] = gx[l] * ux[l] + gy[l] * uy[l];
            f2[l] = gy[l] * ux[l] + gz[l] * uy[l];
        }
        // test functions: sum_i D(i,k) f1(i,l)  +  sum_i D(i,l) f2(k,i)
        Real zz[8];
        octet_contract_any<ASM>(f1, DTk, zz);
#pragma unroll
        for (int l = 0; l < 8; ++l)
        {
            Real s = zz[l];
#pragma unroll
            for (int i = 0; i < 8; ++i)
                s += Dm[i + 8 * l] * f2[i];
            zz[l] = s;
        }
        // assembly across elements.  xi neighbours: column k==7 of ex==0 meets column k==0 of ex==1 (lanes 7|8 of a row)
        if constexpr (ASM && sizeof(Real) == 4)
        {
            const float(&za)[4] = reinterpret_cast<const float(&)[4]>(zz[0]);
            const float(&zb)[4] = reinterpret_cast<const float(&)[4]>(zz[4]);
            float ra[4], rb[4];
            row_neighbours_asm(za, mR, mL, ra);
            row_neighbours_asm(zb, mR, mL, rb);
#pragma unroll
            for (int l = 0; l < 4; ++l)
            {
                z[l] = zz[l] + ra[l];
                z[4 + l] = zz[4 + l] + rb[l];
            }
        }
        else
        {
#pragma unroll
            for (int l = 0; l < 8; ++l)
            {
                const Real from_right = dpp_read<ROW_SHL1>(zz[l]);
                const Real from_left = dpp_read<ROW_SHR1>(zz[l]);
                z[l] = zz[l] + (mR * from_right + mL * from_left);
            }
        }
        // eta neighbours: node l==7 of ey==0 meets node l==0 of ey==1, 16 lanes up
        {
            const Real top = z[7], bottom = z[0];
            const Real from_above = __shfl(bottom, (lane + 16) & 63, 64);
            const Real from_below = __shfl(top, (lane + 48) & 63, 64);
            z[7] = top + mU * from_above;
            z[0] = bottom + mD * from_below;
        }
    }

    // Separable form (kernel 7).  On the rectangles of a uniform_rect mesh the metric is diagonal and a product of 1-D
    // factors, gx(k,l) = alpha_k beta_l, gz(k,l) = gamma_k delta_l, gy = 0, so the sweep  D^T (G (D u))  collapses to
    //     z(k,l) = beta_l * sum_j Ax(k,j) u(j,l)  +  gamma_k * sum_j Ay(l,j) u(k,j),
    // Ax = D^T diag(alpha) D, Ay = D^T diag(delta) D (8 x 8, built in double when the plan is created): ONE contraction
    // per direction instead of two.  Sep = [Ax (k + 8 j): 64 | Ay, packed upper triangle: 36 (+ 28 unused) | beta: 8 | gamma: 8].
    __host__ __device__ constexpr int sym_index(int a, int b) { return a <= b ? a + b * (b + 1) / 2 : b + a * (a + 1) / 2; }

    template <bool ASM, typename Real>
    __device__ inline void wave8_stiffness_sep(const Real (&w)[8], Real (&z)[8], const Real (&AxK)[8], const Real *__restrict__ Sep,
                                               Real gamma, Real mR, Real mL, Real mU, Real mD, int lane)
    {
        // Ay is symmetric: its 36 distinct entries are stored packed (upper triangle, column by column) so that they and
        // beta can stay in scalar registers for the whole time loop
        const Real *Ay = Sep + 64, *beta = Sep + 128;
        Real X[8], zz[8];
        octet_contract_any<ASM>(w, AxK, X);
#pragma unroll
        for (int l = 0; l < 8; ++l)
        {
            Real s = Ay[sym_index(l, 0)] * w[0];
#pragma unroll
            for (int j = 1; j < 8; ++j)
                s += Ay[sym_index(l, j)] * w[j];
            zz[l] = gamma * s + beta[l] * X[l];
        }
        if constexpr (ASM && sizeof(Real) == 4)
        {
            const float(&za)[4] = reinterpret_cast<const float(&)[4]>(zz[0]);
            const float(&zb)[4] = reinterpret_cast<const float(&)[4]>(zz[4]);
            float ra[4], rb[4];
            row_neighbours_asm(za, mR, mL, ra);
            row_neighbours_asm(zb, mR, mL, rb);
#pragma unroll
            for (int l = 0; l < 4; ++l)
            {
                z[l] = zz[l] + ra[l];
                z[4 + l] = zz[4 + l] + rb[l];
            }
        }
        else
        {
#pragma unroll
            for (int l = 0; l < 8; ++l)
            {
                const Real from_right = dpp_read<ROW_SHL1>(zz[l]);
                const Real from_left = dpp_read<ROW_SHR1>(zz[l]);
                z[l] = zz[l] + (mR * from_right + mL * from_left);
            }
        }
        {
            const Real top = z[7], bottom = z[0];
            const Real from_above = __shfl(bottom, (lane + 16) & 63, 64);
            const Real from_below = __shfl(top, (lane + 48) & 63, 64);
            z[7] = top + mU * from_above;
            z[0] = bottom + mD * from_below;
        }
    }

    template <typename Real, bool ASM, bool SEP>
    __global__ void __launch_bounds__(256) ddh_wave8_kernel(DdhArgs<Real> A, const Real *__restrict__ Dmat, const Real *__restrict__ filt,
                                                           const Real *__restrict__ cs, const Real *__restrict__ sn,
                                                           const Real *__restrict__ Sep)
    {
        raise_priority(A.prio);
        const int lane = threadIdx.x & 63;
        const int s_first = A.dom_begin + 2 * (blockIdx.x * 4 + (threadIdx.x >> 6));
        if (s_first >= A.dom_end)
            return; // wave-uniform: the kernel has no barriers
        const int sub = lane >> 5;
        const bool valid = s_first + sub < A.dom_end;
        const int s = domain_at(A, valid ? s_first + sub : s_first); // a missing second subdomain recomputes the first, writes nothing

        const int k = lane & 7, el = (lane >> 3) & 3, ex = el & 1, ey = el >> 1;
        const int fdof = A.s_fdof[s];
        const int *sI = A.sI + 256 * (size_t)s;

        Real gx[8], gy[8], gz[8], invm[8], Hi[8], F[8], Gf[8], u[8], v[8];
#pragma unroll
        for (int l = 0; l < 8; ++l)
        {
            const int node = k + 8 * (l + 8 * el);
            const int d = sI[node];
            if constexpr (!SEP)
            {
                const Real *g = A.G + 3 * ((size_t)node + 256 * (size_t)s);
                gx[l] = g[0];
                gy[l] = g[1];
                gz[l] = g[2];
            }
            else
                gx[l] = gy[l] = gz[l] = 0;
            load_dof(A, s, d, fdof, invm[l], Hi[l], F[l], Gf[l]);
        }

        Real Dk[8], DTk[8];
        Real gamma = 0;
#pragma unroll
        for (int x = 0; x < 8; ++x)
        {
            if constexpr (SEP)
            {
                Dk[x] = Sep[k + 8 * (k ^ x)]; // Ax(k, k^x)
                DTk[x] = 0;
            }
            else
            {
                Dk[x] = Dmat[k + 8 * (k ^ x)];  // D(k, k^x)
                DTk[x] = Dmat[(k ^ x) + 8 * k]; // D(k^x, k)
            }
        }
        if constexpr (SEP)
            gamma = Sep[136 + k];
        const Real mR = (k == 7 && ex == 0) ? Real(1) : Real(0);
        const Real mL = (k == 0 && ex == 1) ? Real(1) : Real(0);
        const Real mU = (ey == 0) ? Real(1) : Real(0);
        const Real mD = (ey == 1) ? Real(1) : Real(0);

        auto sweep = [&](const Real(&w)[8], Real(&z)[8])
        {
            if constexpr (SEP)
                wave8_stiffness_sep<ASM>(w, z, Dk, Sep, gamma, mR, mL, mU, mD, lane);
            else
                wave8_stiffness<ASM>(w, z, gx, gy, gz, Dk, DTk, Dmat, mR, mL, mU, mD, lane);
        };
        wh_march(A, A.nt, A.dt, filt, cs, sn, invm, Hi, F, Gf, u, v, sweep);

        if (!valid)
            return;
#pragma unroll
        for (int l = 0; l < 8; ++l)
        {
            // every shared node is held by 2 or 4 (lane, l) pairs with identical values: the copy with
            // the smallest element-node index writes
            const bool owner = !(k == 0 && ex > 0) && !(l == 0 && ey > 0);
            if (owner)
                publish_dof(A, s, sI[k + 8 * (l + 8 * el)], fdof, u[l], v[l], false);
        }
    }

    // ---------------------------------------------------------------- kernels 5 and 8: dense element matrix on the matrix cores (NB = 4, uniform geometry)
    // When every element of every subdomain has the same metric tensor (always the case on the uniform_rect
    // meshes DDH supports) the element-local part of a stiffness sweep is Z = K U with one 16x16 element matrix K
    // and U = (16 nodes) x (16 elements of the subdomain): exactly one 16x16x16 product, i.e. four
    // v_mfma_f32_16x16x4_f32 (kernel 5, Real = float) or v_mfma_f64_16x16x4_f64 (kernel 8, Real = double) per sweep on the
    // matrix pipe, leaving the VALU only the assembly and the RK2 update.
    // Lane = element + 16 g, and register r of a lane holds element node node_of(g, r): the nodes are numbered by CLASS, not
    // by eta index.  Register 0 = the four element-interior nodes, 1 = the xi-face nodes (xi index 0 or 3, eta index 1 or 2),
    // 2 = the eta-face nodes, 3 = the corners; bit 0 of g picks the low / high xi side, bit 1 the eta side.  The matrix
    // instruction does not care how the 16 nodes are numbered: the B operand of step st takes row kk = 4 st + (lane >> 4) from
    // register st, i.e. node (g, r = st), and the C/D map returns row 4 (lane >> 4) + reg (fp32) or (lane >> 4) + 4 reg
    // (fp64), so with K's columns ordered 4 r + g and its rows 4 g + r (fp32) or g + 4 r (fp64), build_dense_element_matrix,
    // the result lands where the input was.  What the numbering buys is in the vector work around the matrix instructions:
    //   * register 0 is shared with no other element: no assembly.  It is never a trace dof (checked when the plan is built,
    //     ddh_interior_check_kernel): no Hi term, and without x no sources (wh_march's LEAN);
    //   * register 1 needs the xi neighbour only, register 2 the eta neighbour only, register 3 both, xi first and eta on the
    //     result, so every copy of a shared node forms the same commutative sums and stays bitwise equal to its twins;
    //   * the xi partner of (el, g) is (el +- 1, g ^ 1), the eta partner (el +- 4, g ^ 2), the same lanes for both registers
    //     of a direction: four ds_bpermute and four masked FMAs per sweep (before: four ds_bpermute, two DPP moves, six FMAs).
    // In fp64 K is formed and kept in double: every operation of a sweep is fp64, the summation order alone differs from the
    // sum-factorised kernels 1 and 2.
    // On gfx950 the f32 MFMA runs at the vector rate and does not overlap with VALU work, so what counts is the
    // number of issue cycles: 4 MFMAs (128 cycles) replace the ~80 VALU instructions (160 cycles + DPP hazards) of the
    // sum-factorised sweep, and the xi-neighbour exchange goes through ds_bpermute (LDS pipe, no VALU slots); a
    // variant with odd elements stored mirrored in xi so that every exchange is a DPP row shift measured 24 % slower
    // (96 instead of 72 VALU instructions per time step).
    // PRIO: the four matrix instructions of a sweep are issued with priority over the other resident wavefronts' vector work.
    // The fp32 matrix instructions run on the SIMD's own fp32 lanes (no co-execution with VALU: SQ_VALU_MFMA_COEXEC_CYCLES = 0,
    // profiles/r03/pmc_ddh_kernel5_coexec.txt, mfma_valu_coexec.txt) and a vector instruction issued behind a matrix
    // instruction waits for its passes to drain, so grouping the wavefronts' matrix instructions saves issue cycles
    // (same-box A/B, 16,384 subdomains: 85.2 -> 83.4 ms per action; order of issue only, results bitwise unchanged): on in
    // fp32.  In fp64 that grouping is 0.7-1.7 % slower than plain issue order (same-box A/B, profiles/r04/ddh64_prio_ab.txt),
    // hence off unless built with CUDDH_DDH64_MFMA_PRIO=1; the knob stays for A/B builds (profiles/tools/build_variant.py).
#ifndef CUDDH_DDH64_MFMA_PRIO
#define CUDDH_DDH64_MFMA_PRIO 0
#endif
    typedef float f4 __attribute__((ext_vector_type(4)));
    typedef double d4 __attribute__((ext_vector_type(4)));
    __device__ inline f4 mfma_16x16x4(float a, float b, f4 acc) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0); }
    __device__ inline d4 mfma_16x16x4(double a, double b, d4 acc) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0); }

    // element node (xi index k, eta index l), as k + 4 l, held by register r of the lanes with lane >> 4 == g
    __host__ __device__ constexpr int node_of(int g, int r)
    {
        const int k = (r & 1) ? 3 * (g & 1) : 1 + (g & 1), l = (r & 2) ? 3 * (g >> 1) : 1 + (g >> 1);
        return k + 4 * l;
    }

    // FORCED: x is given (rhs, postprocess), so dofs that are no trace dofs carry sources too.  HOLD: the launch holds issue
    // priority as a whole (A.prio, multi-GPU boundary subdomains) and the sweeps do not give it back.  Both are properties of
    // a launch and template parameters so that the time loop has no branch on them.
    template <typename Real, bool FORCED, bool HOLD, typename... Grids>
    __global__ void __launch_bounds__(256) ddh_mfma_kernel(DdhArgs<Real> A, const Real *__restrict__ Aop, const Real *__restrict__ filt,
                                                          const Real *__restrict__ cs, const Real *__restrict__ sn, Grids... grids)
    {
        constexpr bool PRIO = sizeof(Real) == 4 || CUDDH_DDH64_MFMA_PRIO;
        typedef Real r4 __attribute__((ext_vector_type(4)));
        const int lane = threadIdx.x & 63;
        const int position = A.dom_begin + blockIdx.x * 4 + (threadIdx.x >> 6);
        if (position >= A.dom_end)
            return; // wave-uniform, no barriers in this kernel
        const int s = domain_at(A, position, grids...);
        if constexpr (HOLD)
            __builtin_amdgcn_s_setprio(3);

        const int g = lane >> 4, el = lane & 15, ex = el & 3, ey = el >> 2;
        const int fdof = A.s_fdof[s];
        const int *sI = A.sI + 256 * (size_t)s;

        Real invm[4], Hi[4], F[4], Gf[4], u[4], v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
            load_dof(A, s, sI[node_of(g, r) + 16 * el], fdof, invm[r], Hi[r], F[r], Gf[r]);
        Real Ka[4];
#pragma unroll
        for (int st = 0; st < 4; ++st)
            Ka[st] = Aop[64 * st + lane];

        // neighbours: the high xi side of element ex meets the low xi side of element ex + 1 (g ^ 1), and the same in eta
        // with el + 4 and g ^ 2.  A lane without a neighbour reads itself and masks the value out.
        const bool hiX = g & 1, hiY = g >> 1;
        const bool hasX = hiX ? ex < 3 : ex > 0, hasY = hiY ? ey < 3 : ey > 0;
        const int pX = hasX ? (hiX ? el + 1 : el - 1) + 16 * (g ^ 1) : lane;
        const int pY = hasY ? (hiY ? el + 4 : el - 4) + 16 * (g ^ 2) : lane;
        const Real mX = hasX ? Real(1) : Real(0), mY = hasY ? Real(1) : Real(0);

        auto sweep = [&](const Real(&w)[4], Real(&z)[4])
        {
            r4 acc = {0, 0, 0, 0};
            if constexpr (PRIO && !HOLD)
                __builtin_amdgcn_s_setprio(3);
#pragma unroll
            for (int st = 0; st < 4; ++st)
                acc = mfma_16x16x4(Ka[st], w[st], acc);
            if constexpr (PRIO && !HOLD)
                __builtin_amdgcn_s_setprio(0);
            const Real x1 = __shfl(acc[1], pX, 64), x3 = __shfl(acc[3], pX, 64), y2 = __shfl(acc[2], pY, 64);
            z[0] = acc[0];
            z[1] = acc[1] + mX * x1;
            z[2] = acc[2] + mY * y2;
            const Real c = acc[3] + mX * x3;
            z[3] = c + mY * __shfl(c, pY, 64);
        };
        const TimeGridView<Real> tg = time_grid_of(A, s, filt, cs, sn, grids...);
        wh_march<FORCED ? 2 : 1, 1u, scheme_of<Grids...>>(A, tg.nt, tg.dt, tg.filt, tg.cs, tg.sn, invm, Hi, F, Gf, u, v, sweep);

#pragma unroll
        for (int r = 0; r < 4; ++r)
        {
            // every shared node is held by 2 or 4 (lane, register) pairs with identical values: the copy with
            // the smallest element-node index writes
            const int n = node_of(g, r), k = n & 3, l = n >> 2;
            const bool owner = !(k == 0 && ex > 0) && !(l == 0 && ey > 0);
            if (owner)
                publish_dof(A, s, sI[n + 16 * el], fdof, u[r], v[r], false);
        }
    }

    // ---------------------------------------------------------------- kernel 5, element-lane form (NB = 4, rectangles): four subdomains per wavefront
    // On rectangles the element matrix is a sum of two Kronecker terms (the separable form of kernel 7),
    //     z(k,l) = beta_l sum_j Ax(k,j) w(j,l) + gamma_k sum_j Ay(l,j) w(k,j):
    // 7 non-zeros per row where the dense product of ddh_mfma_kernel multiplies 16.  Lane = one whole ELEMENT, ex + 4 ey, one
    // subdomain per 16-lane row, four subdomains per wavefront; register n = k + 4 l holds the element's node (k, l).  Both
    // contractions are then in-lane full-rate FMAs with scalar-register coefficients, and the matrix pipe and LDS are not
    // used.  To keep the coefficients within the scalar registers the node weight W(k,l) = gamma_k beta_l is factored out of
    // both terms, z = W z',
    //     z'(k,l) = Dg(k,l) w(k,l) + sum_{j != k} Bx(k,j) w(j,l) + sum_{j != l} By(l,j) w(k,j),
    // Bx = Ax / gamma_k, By = Ay / beta_l, Dg = Bx(k,k) + By(l,l): 12 + 12 + 16 scalars.  All copies of a shared dof carry
    // the same W (checked when the plan is built), so the assembled sum is W sum z' and W moves into the per-dof constants:
    // invm is multiplied by it, Hi, F and Gf are divided.  Assembly is the only cross-lane work: xi neighbours are lane +- 1,
    // eta neighbours lane +- 4, DPP row shifts that never leave the 16-lane row, so a subdomain's result does not depend on
    // its wave-mates.  xi first and eta on the result; the copies of a shared node hold one sum, rounded once, and stay
    // bitwise equal.  Registers with k, l in {1, 2} are element-interior: wh_march's LEAN rules apply to them.
    // A launch whose length is no multiple of 4 is handled as ddh_wave8_kernel handles its odd tail: the missing rows
    // recompute the wavefront's first subdomain and publish nothing.
    // The time loop runs on register pairs (below, "the packed form"): two nodes per v_pk_fma_f32, 262 vector instructions
    // per wavefront-step in the action form where the node-by-node loop issued 440 (264 with LAST_COPY, 273 / 272 with x against
    // 456), bitwise the same results (profiles/r16, profiles/r17).  PAIRED (chain order 2, cuddh_hip_ddh_plan_set_chain_order;
    // what auto runs where auto chose this form) sums a node's seven terms in another order, in which both halves of a pair
    // meet every term at the same place (element_lane_pair_product): 56 packed instructions per sweep instead of 71, all
    // eight pairs keep dm, 228 per wavefront-step in the action form (244 with x), 164 VGPRs, no scratch; a new rounding,
    // gated against the fp64 oracle and not against the pinned chains' bits (profiles/r22).  The one-grid kernel only: the
    // TimeGrids instantiations (kernel 13) and a form forced with set_sweep_form keep the pinned chains.
    // Every form is compiled for three wavefronts per SIMD with no scratch: 168 VGPRs in the action form, 166 / 167 in
    // the form with x (rhs, postprocess: once per solve).  The assembly is 16 DPP instructions per sweep with no mask
    // multiplications in eta and one mask in xi (element_assemble_*_row_asm below): a shared node's sum is formed by one
    // copy and moved to the other, and a lane without the neighbour is not written; the masked form with the DPP reads
    // folded into the arithmetic (CUDDH_EL_ASSEMBLE, 12 per call) stays for kernel 11's xi direction.  Measured at 65,536 subdomains, ms per
    // action, for the masked form (profiles/r08/element_lane_variants.txt):
    // two wavefronts and dpp_read + FMA 271.3, three wavefronts 268.2, folded 265.7, both 258.6; the matrix form 273.9.
    // LAST_COPY (cuddh_hip_ddh_plan_set_sweep_form(plan, 3)) turns the owner rule round, so that a test can see the other
    // copies: the results are bitwise the same.
    // Assembly of four node pairs with the cross-lane reads folded into the arithmetic :
    // hi[i] += mHi * (lo[i] of lane + SHIFT), lo[i] += mLo * (hi[i] of lane - SHIFT), both from the values before the call.
    // 12 instructions where the plain form has 8 v_mov_b32_dpp and 8 FMAs; the masks are 0 or 1, so the sums are the same.
#define CUDDH_EL_ASSEMBLE(NAME, SHL, SHR)                                                                                                  \
    __device__ inline void NAME(float (&hi)[4], float (&lo)[4], float mHi, float mLo)                                                      \
    {                                                                                                                                      \
        float t0, t1, t2, t3;                                                                                                              \
        asm volatile("s_nop 1\n\t"                                                                                                         \
                     "v_mul_f32_dpp %8, %0, %13 " SHR " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"                                       \
                     "v_mul_f32_dpp %9, %1, %13 " SHR " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"                                       \
                     "v_mul_f32_dpp %10, %2, %13 " SHR " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"                                      \
                     "v_mul_f32_dpp %11, %3, %13 " SHR " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"                                      \
                     "v_fmac_f32_dpp %0, %4, %12 " SHL " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"                                      \
                     "v_fmac_f32_dpp %1, %5, %12 " SHL " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"                                      \
                     "v_fmac_f32_dpp %2, %6, %12 " SHL " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"                                      \
                     "v_fmac_f32_dpp %3, %7, %12 " SHL " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"                                      \
                     "v_add_f32 %4, %4, %8\n\t"                                                                                            \
                     "v_add_f32 %5, %5, %9\n\t"                                                                                            \
                     "v_add_f32 %6, %6, %10\n\t"                                                                                           \
                     "v_add_f32 %7, %7, %11\n\t"                                                                                           \
                     : "+v"(hi[0]), "+v"(hi[1]), "+v"(hi[2]), "+v"(hi[3]), "+v"(lo[0]), "+v"(lo[1]), "+v"(lo[2]), "+v"(lo[3]), "=&v"(t0),   \
                       "=&v"(t1), "=&v"(t2), "=&v"(t3)                                                                                     \
                     : "v"(mHi), "v"(mLo));                                                                                                \
    }
    CUDDH_EL_ASSEMBLE(element_assemble_xi_asm, "row_shl:1", "row_shr:1")
#undef CUDDH_EL_ASSEMBLE
    // The assembly of ddh_element_lane_kernel, where a 16-lane DPP row is one subdomain (kernel 11's rows hold two eta-rows
    // and keep the masked form above).  The two copies of a shared node need the same sum: one copy forms it, the other
    // takes it with a DPP move, and a lane without that neighbour is left unwritten instead of adding 0 * y.  8 DPP
    // instructions per call where the masked form has 8 and 4 v_add_f32, no temporaries, and the value of every written
    // lane is the one rounded sum it was before (x + 0 * y against x: the same for finite y, up to the sign of a zero).
    // eta, lane +- 4: without bound_ctrl a lane whose source lies outside the row is not written, which is ey == 3 for
    // row_shl:4 and ey == 0 for row_shr:4, so no mask operand at all.  up[i] += dn[i] of lane + 4; dn[i] = that sum of
    // lane - 4.  A DPP read needs two wait states after the vector write of its source: the s_nop for the values the
    // compiler wrote last, three instructions between each add and the move that reads it.
    __device__ inline void element_assemble_eta_row_asm(float (&up)[4], float (&dn)[4])
    {
        asm volatile("s_nop 1\n\t"
                     "v_add_f32_dpp %0, %4, %0 row_shl:4 row_mask:0xf bank_mask:0xf\n\t"
                     "v_add_f32_dpp %1, %5, %1 row_shl:4 row_mask:0xf bank_mask:0xf\n\t"
                     "v_add_f32_dpp %2, %6, %2 row_shl:4 row_mask:0xf bank_mask:0xf\n\t"
                     "v_add_f32_dpp %3, %7, %3 row_shl:4 row_mask:0xf bank_mask:0xf\n\t"
                     "v_mov_b32_dpp %4, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                     "v_mov_b32_dpp %5, %1 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                     "v_mov_b32_dpp %6, %2 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                     "v_mov_b32_dpp %7, %3 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                     : "+v"(up[0]), "+v"(up[1]), "+v"(up[2]), "+v"(up[3]), "+v"(dn[0]), "+v"(dn[1]), "+v"(dn[2]), "+v"(dn[3]));
    }
    // xi, lane +- 1: the lanes to leave out are ex == 3 and ex == 0, every fourth lane, which neither bound_ctrl nor
    // bank_mask (four consecutive lanes) can name.  hi[i] += mHi * (lo[i] of lane + 1) as in the masked form; lo[i] = that
    // sum of lane - 1 unless VCC holds the lane (ex == 0), through v_cndmask_b32_dpp (D = VCC ? src1 : DPP(src0)).  VCC is
    // set inside the statement, by scalar instructions (no wait states before a vector read of it); they also stand between
    // the compiler's last vector write and the first DPP read.
    __device__ inline void element_assemble_xi_row_asm(float (&hi)[4], float (&lo)[4], float mHi)
    {
        asm volatile("s_mov_b32 vcc_lo, 0x11111111\n\t"
                     "s_mov_b32 vcc_hi, 0x11111111\n\t"
                     "v_fmac_f32_dpp %0, %4, %8 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %1, %5, %8 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %2, %6, %8 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %3, %7, %8 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_cndmask_b32_dpp %4, %0, %4, vcc row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                     "v_cndmask_b32_dpp %5, %1, %5, vcc row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                     "v_cndmask_b32_dpp %6, %2, %6, vcc row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                     "v_cndmask_b32_dpp %7, %3, %7, vcc row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                     : "+v"(hi[0]), "+v"(hi[1]), "+v"(hi[2]), "+v"(hi[3]), "+v"(lo[0]), "+v"(lo[1]), "+v"(lo[2]), "+v"(lo[3])
                     : "v"(mHi)
                     : "vcc");
    }
    // The same two for the five values a side of an n_basis-5 element holds (ddh_element_lane5_kernel): the same instructions,
    // one more of each, so four instructions stand between a sum and the move that reads it.
    __device__ inline void element_assemble_eta_row5_asm(float (&up)[5], float (&dn)[5])
    {
        asm volatile("s_nop 1\n\t"
                     "v_add_f32_dpp %0, %5, %0 row_shl:4 row_mask:0xf bank_mask:0xf\n\t"
                     "v_add_f32_dpp %1, %6, %1 row_shl:4 row_mask:0xf bank_mask:0xf\n\t"
                     "v_add_f32_dpp %2, %7, %2 row_shl:4 row_mask:0xf bank_mask:0xf\n\t"
                     "v_add_f32_dpp %3, %8, %3 row_shl:4 row_mask:0xf bank_mask:0xf\n\t"
                     "v_add_f32_dpp %4, %9, %4 row_shl:4 row_mask:0xf bank_mask:0xf\n\t"
                     "v_mov_b32_dpp %5, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                     "v_mov_b32_dpp %6, %1 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                     "v_mov_b32_dpp %7, %2 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                     "v_mov_b32_dpp %8, %3 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                     "v_mov_b32_dpp %9, %4 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
                     : "+v"(up[0]), "+v"(up[1]), "+v"(up[2]), "+v"(up[3]), "+v"(up[4]), "+v"(dn[0]), "+v"(dn[1]), "+v"(dn[2]), "+v"(dn[3]),
                       "+v"(dn[4]));
    }
    __device__ inline void element_assemble_xi_row5_asm(float (&hi)[5], float (&lo)[5], float mHi)
    {
        asm volatile("s_mov_b32 vcc_lo, 0x11111111\n\t"
                     "s_mov_b32 vcc_hi, 0x11111111\n\t"
                     "v_fmac_f32_dpp %0, %5, %10 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %1, %6, %10 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %2, %7, %10 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %3, %8, %10 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_fmac_f32_dpp %4, %9, %10 row_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                     "v_cndmask_b32_dpp %5, %0, %5, vcc row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                     "v_cndmask_b32_dpp %6, %1, %6, vcc row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                     "v_cndmask_b32_dpp %7, %2, %7, vcc row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                     "v_cndmask_b32_dpp %8, %3, %8, vcc row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                     "v_cndmask_b32_dpp %9, %4, %9, vcc row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                     : "+v"(hi[0]), "+v"(hi[1]), "+v"(hi[2]), "+v"(hi[3]), "+v"(hi[4]), "+v"(lo[0]), "+v"(lo[1]), "+v"(lo[2]), "+v"(lo[3]),
                       "+v"(lo[4])
                     : "v"(mHi)
                     : "vcc");
    }
    constexpr unsigned ELEMENT_INTERIOR_REGISTERS = (1u << 5) | (1u << 6) | (1u << 9) | (1u << 10);

    // the in-lane part of the element-lane sweep: z' = Dg w + Bx-terms + By-terms of the lane's own element, before assembly
    __device__ inline void element_lane_products(const float (&w)[16], float (&z)[16], const float (&Bx)[16], const float (&By)[16],
                                                 const float (&Dg)[16])
    {
#pragma unroll
        for (int l = 0; l < 4; ++l)
#pragma unroll
            for (int k = 0; k < 4; ++k)
            {
                float t = Dg[k + 4 * l] * w[k + 4 * l];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                {
                    if (j != k)
                        t += Bx[k + 4 * j] * w[j + 4 * l];
                    if (j != l)
                        t += By[l + 4 * j] * w[k + 4 * j];
                }
                z[k + 4 * l] = t;
            }
    }

    // ---- the packed form of the above (ddh_element_lane_kernel only): two nodes per 64-bit register pair, v_pk_fma_f32
    // The loop is bound by the number of vector instructions it issues, and a v_pk_fma_f32 costs one issue for
    // two FMAs.  Pair P = k + 4 h holds the nodes (k, l_a) in .x and (k, l_b) in .y, (l_a, l_b) = (0, 3) for h = 0 and (1, 2)
    // for h = 1: the element-interior registers {5, 6, 9, 10} are the whole pairs 5 and 6, and the halves the assembly works
    // on are plain 32-bit registers of the pairs.  Every half runs the chain of fp32 FMAs that element_lane_products and
    // wh_march run for its node, written as explicit FMAs, so the results are bitwise the same -- with one change that is
    // exact: the pairs keep hm = half_dt invm alone and not dm = dt invm = 2 hm beside it, and q += dm dq is computed as
    // q += hm (dq + dq).  Doubling is exact in binary floating point (short of overflow, and of a subnormal hm, neither of
    // which a stable local solve comes near), so hm (dq + dq) is the same real number as dm dq and the FMA rounds it the
    // same.  It costs a v_pk_add_f32 per pair and step and frees two registers per pair: with dm for all eight the pairs
    // need 174 at the widest point of the second sweep (a pair of the input dies only when five pairs of the result are
    // complete, where single registers need seven) and the loop spills at three wavefronts per SIMD.  The assembly without
    // mask registers and temporaries (element_assemble_*_row_asm) left room for dm in five pairs of the action form and in
    // two of the form with x (ELEMENT_LANE_DM_PAIRS); the other pairs double dq.
    // Scalar registers: the coefficients are operands of the packed instruction as aligned pairs, By and Dg as the pairs
    // the halves need, the 12 off-diagonal Bx two to a pair with op_sel choosing the half (as a broadcast scalar of its
    // own each would take a pair); 106 are in use and none is spilled inside the time loop (a dozen wait in the lanes of
    // one vector register across it and come back once per WaveHoltz iteration).
    typedef float pair_t __attribute__((ext_vector_type(2)));
    constexpr int el_pair(int k, int l) { return k + 4 * ((l == 1 || l == 2) ? 1 : 0); }
    constexpr int el_half(int l) { return l >= 2 ? 1 : 0; }
    constexpr unsigned ELEMENT_INTERIOR_PAIRS = (1u << 5) | (1u << 6);
    // the pairs that keep dm beside hm (wh_march_pairs' DM): as many as fit 168 vector registers, three wavefronts per SIMD,
    // with no scratch; which pairs does not matter to the count (profiles/r17/ddh_codegen_compare.txt)
    constexpr unsigned ELEMENT_LANE_DM_PAIRS(bool forced) { return forced ? 0x60u : 0x1fu; }
    // the same for the paired chains (element_lane_pair_product<K, H, true>), chosen again: without the head temporaries all
    // eight pairs of the action form keep dm at 164 registers and its three v_pk_add_f32 go; the form with x spills from
    // three pairs on and keeps the two interior ones (profiles/r22/ddh_codegen_compare.txt lists the masks tried)
    constexpr unsigned ELEMENT_LANE_PAIRED_DM_PAIRS(bool forced) { return forced ? 0x60u : 0xffu; }

    __device__ inline pair_t pk_fma(pair_t a, pair_t b, pair_t c) { return __builtin_elementwise_fma(a, b, c); }
    __device__ inline pair_t pk_fma(float a, pair_t b, pair_t c) { return __builtin_elementwise_fma(pair_t{a, a}, b, c); }
    // t += (half HALF of the scalar-register pair c, in both halves) * w: two coefficients share an aligned pair of scalar
    // registers (the compiler keeps a broadcast scalar of the time loop as a pair of its own with both halves the same)
    template <int HALF>
    __device__ inline void pk_fmac_scalar(pair_t &t, pair_t c, pair_t w)
    {
        if constexpr (HALF == 0)
            asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]" : "+v"(t) : "s"(c), "v"(w));
        else
            asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(t) : "s"(c), "v"(w));
    }
    // where the off-diagonal Bx(k, j) waits: half bx_slot % 2 of pair bx_slot / 2
    constexpr int bx_slot(int k, int j) { return 3 * k + (j < k ? j : j - 1); }
    // t += c * (half HALF of w, in both halves): the compiler broadcasts the low half through op_sel_hi but copies the high
    // half into a pair of its own first, so op_sel is written here
    template <int HALF>
    __device__ inline void pk_fmac_half(pair_t &t, pair_t c, pair_t w)
    {
        if constexpr (HALF == 0)
            asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(t) : "s"(c), "v"(w));
        else
            asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "+v"(t) : "s"(c), "v"(w));
    }

    // t = c * (half HALF of w, in both halves)
    template <int HALF>
    __device__ inline pair_t pk_mul_half(pair_t c, pair_t w)
    {
        pair_t t;
        if constexpr (HALF == 0)
            asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(t) : "s"(c), "v"(w));
        else
            asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(t) : "s"(c), "v"(w));
        return t;
    }
    // t.x += c.x * w.y, t.y += c.y * w.x: the halves of w crossed, the coefficient pair straight (the compiler copies a high
    // half into a pair of its own otherwise, as in pk_fmac_half)
    __device__ inline void pk_fmac_crossed(pair_t &t, pair_t c, pair_t w)
    {
        asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,0,1]" : "+v"(t) : "s"(c), "v"(w));
    }

    // element_lane_products on pairs.  A node's chain is Dg w, then for j = 0..3 the x-term (j != k) and the y-term (j != l).
    // The x-term has one coefficient for both halves.  The y-term has the coefficient pair (By(l_a,j), By(l_b,j)) and
    // w(k,j) from one half of pair (k, h_j); for j == l_a or l_b that is the pair itself, and only the other half has
    // the term: one v_fmac_f32 on that half, at its place in the chain.  8 instructions per pair where the nodes took 14.
    // The head of the chain: t = Dg w; t += c w' adds two products, and of the two the compiler of the node-by-node loop
    // (element_lane_products under -ffp-contract=fast, read from its code object: the same in both sweeps and in all
    // forms of the kernel) rounds c w' and fuses Dg w on the seven nodes with k == 0 or l == 0, and rounds Dg w and fuses
    // c w' on the other nine.  The results are compared bitwise with that loop's, so the choice is kept node by node:
    //   k != 0, pairs (1, 2):  Dg w rounded in both halves;
    //   k != 0, pairs (0, 3):  the half l = 0 rounds Bx(k,0) w(0,0) instead: one multiplication and one FMA on that half
    //                          replace what the two packed instructions leave there;
    //   k == 0, pairs (1, 2):  both halves round the y-term of j = 0, By(l,0) w(0,0): packed;
    //   k == 0, pairs (0, 3):  the half l = 0 rounds its x-term of j = 1 and the half l = 3 its y-term of j = 0: two
    //                          multiplications, then Dg w packed, then the x-term of j = 1 on the half l = 3 alone.
    // 71 instructions per sweep (64 + 2 for each of three pairs + 1).
    //
    // PAIRED, the paired chains (chain order 2, cuddh_hip_ddh_plan_set_chain_order): another summation order of the same
    // seven terms per node, one rounded product and six FMAs, in which both halves of a pair meet every term at the same
    // place, so that every instruction is a packed one.  For pair P = K + 4 H, Q = K + 4 (1 - H), (l_a, l_b) = (H, 3 - H):
    //   1. t = Dg[P] w[P], rounded in both halves (one v_pk_mul_f32; no head rules);
    //   2. for j = 0, 1, 2, 3 in this order: the x-term Bx(K,j) w(j,l) if j != K, then the y-term (By(l_a,j), By(l_b,j)) w(K,j)
    //      if j is neither l_a nor l_b (w(K,j) is a half of w[Q]);
    //   3. last the two y-terms that read the pair itself, crossed: .x += By(l_a,l_b) w[P].y, .y += By(l_b,l_a) w[P].x, one
    //      v_pk_fma_f32 with op_sel crossing the halves of w[P] (pk_fmac_crossed).
    // The pinned chains take each of the two crossed terms at j = l_b (low half) and j = l_a (high half), which are different
    // places; moving both to the end is what lets them share an instruction.  7 instructions per pair, 56 per sweep.  By is
    // six aligned scalar pairs: (By(l_a,j), By(l_b,j)) for the two j outside {l_a, l_b} and the crossed pair, per H.
    template <int K, int H, bool PAIRED = false>
    __device__ inline pair_t element_lane_pair_product(const pair_t (&w)[8], const pair_t (&Bx)[6], const float (&By)[16], const pair_t (&Dg)[8])
    {
        constexpr int la = H, lb = 3 - H, P = K + 4 * H, Q = K + 4 * (1 - H);
        pair_t t;
        if constexpr (PAIRED)
        {
            t = Dg[P] * w[P];
            // j = 0
            if constexpr (K != 0)
                pk_fmac_scalar<bx_slot(K, 0) % 2>(t, Bx[bx_slot(K, 0) / 2], w[0 + 4 * H]);
            if constexpr (H == 1)
                pk_fmac_half<el_half(0)>(t, pair_t{By[la + 0], By[lb + 0]}, w[Q]);
            // j = 1
            if constexpr (K != 1)
                pk_fmac_scalar<bx_slot(K, 1) % 2>(t, Bx[bx_slot(K, 1) / 2], w[1 + 4 * H]);
            if constexpr (H == 0)
                pk_fmac_half<el_half(1)>(t, pair_t{By[la + 4], By[lb + 4]}, w[Q]);
            // j = 2
            if constexpr (K != 2)
                pk_fmac_scalar<bx_slot(K, 2) % 2>(t, Bx[bx_slot(K, 2) / 2], w[2 + 4 * H]);
            if constexpr (H == 0)
                pk_fmac_half<el_half(2)>(t, pair_t{By[la + 8], By[lb + 8]}, w[Q]);
            // j = 3
            if constexpr (K != 3)
                pk_fmac_scalar<bx_slot(K, 3) % 2>(t, Bx[bx_slot(K, 3) / 2], w[3 + 4 * H]);
            if constexpr (H == 1)
                pk_fmac_half<el_half(3)>(t, pair_t{By[la + 12], By[lb + 12]}, w[Q]);
            // the pair's own halves, crossed
            pk_fmac_crossed(t, pair_t{By[la + 4 * lb], By[lb + 4 * la]}, w[P]);
            return t;
        }
        // the head, through j = 0 (and for K == 0, H == 0 the x-term of j = 1)
        if constexpr (K != 0 && H == 1)
        {
            t = Dg[P] * w[P];
            pk_fmac_scalar<bx_slot(K, 0) % 2>(t, Bx[bx_slot(K, 0) / 2], w[0 + 4 * H]);
            pk_fmac_half<0>(t, pair_t{By[la + 0], By[lb + 0]}, w[Q]);
        }
        else if constexpr (K != 0 && H == 0)
        {
            const float first = Bx[bx_slot(K, 0) / 2][bx_slot(K, 0) % 2] * w[0 + 4 * H].x;
            t = Dg[P] * w[P]; // these two are for the half l = 3 (.y) alone ...
            pk_fmac_scalar<bx_slot(K, 0) % 2>(t, Bx[bx_slot(K, 0) / 2], w[0 + 4 * H]);
            t.x = __builtin_fmaf(Dg[P].x, w[P].x, first); // ... what they left in .x is replaced: the half l = 0 has the other order
            t.y = __builtin_fmaf(By[lb + 0], w[P].x, t.y);
        }
        else if constexpr (K == 0 && H == 1)
        {
            t = pk_mul_half<0>(pair_t{By[la + 0], By[lb + 0]}, w[Q]);
            t = pk_fma(Dg[P], w[P], t);
        }
        else
        {
            t.x = Bx[bx_slot(K, 1) / 2][bx_slot(K, 1) % 2] * w[1 + 4 * H].x;
            t.y = By[lb + 0] * w[P].x;
            t = pk_fma(Dg[P], w[P], t);
            t.y = __builtin_fmaf(Bx[bx_slot(K, 1) / 2][bx_slot(K, 1) % 2], w[1 + 4 * H].y, t.y);
        }
        // j = 1
        if constexpr (K != 1 && !(K == 0 && H == 0))
            pk_fmac_scalar<bx_slot(K, 1) % 2>(t, Bx[bx_slot(K, 1) / 2], w[1 + 4 * H]);
        if constexpr (H == 1)
            t.y = __builtin_fmaf(By[lb + 4], w[P].x, t.y);
        else
            pk_fmac_half<0>(t, pair_t{By[la + 4], By[lb + 4]}, w[Q]);
        // j = 2
        if constexpr (K != 2)
            pk_fmac_scalar<bx_slot(K, 2) % 2>(t, Bx[bx_slot(K, 2) / 2], w[2 + 4 * H]);
        if constexpr (H == 1)
            t.x = __builtin_fmaf(By[la + 8], w[P].y, t.x);
        else
            pk_fmac_half<1>(t, pair_t{By[la + 8], By[lb + 8]}, w[Q]);
        // j = 3
        if constexpr (K != 3)
            pk_fmac_scalar<bx_slot(K, 3) % 2>(t, Bx[bx_slot(K, 3) / 2], w[3 + 4 * H]);
        if constexpr (H == 0)
            t.x = __builtin_fmaf(By[la + 12], w[P].y, t.x);
        else
            pk_fmac_half<1>(t, pair_t{By[la + 12], By[lb + 12]}, w[Q]);
        return t;
    }

    template <bool PAIRED = false>
    __device__ inline void element_lane_products_packed(const pair_t (&w)[8], pair_t (&z)[8], const pair_t (&Bx)[6], const float (&By)[16],
                                                        const pair_t (&Dg)[8])
    {
        z[0] = element_lane_pair_product<0, 0, PAIRED>(w, Bx, By, Dg);
        z[1] = element_lane_pair_product<1, 0, PAIRED>(w, Bx, By, Dg);
        z[2] = element_lane_pair_product<2, 0, PAIRED>(w, Bx, By, Dg);
        z[3] = element_lane_pair_product<3, 0, PAIRED>(w, Bx, By, Dg);
        z[4] = element_lane_pair_product<0, 1, PAIRED>(w, Bx, By, Dg);
        z[5] = element_lane_pair_product<1, 1, PAIRED>(w, Bx, By, Dg);
        z[6] = element_lane_pair_product<2, 1, PAIRED>(w, Bx, By, Dg);
        z[7] = element_lane_pair_product<3, 1, PAIRED>(w, Bx, By, Dg);
    }

    // wh_march's RK2 loop in its LEAN forms on pairs: the same expressions with the fusions -ffp-contract=fast gives them
    // in wh_march written out, so they do not depend on it.  INTERIOR holds a bit per pair, and so does DM: a pair with its
    // bit set keeps dm = dt invm beside hm and ends the step with q += dm dq, as wh_march does, the others with
    // q += hm (dq + dq) (above).
    template <int LEAN, unsigned INTERIOR, unsigned DM, int N, typename Sweep>
    __device__ inline void wh_march_pairs(const DdhArgs<float> &A, const int nt, const float dt, const float *__restrict__ filt,
                                          const float *__restrict__ cs, const float *__restrict__ sn, const pair_t (&invm)[N],
                                          const pair_t (&Hi)[N], const pair_t (&F)[N], const pair_t (&Gf)[N], pair_t (&u)[N], pair_t (&v)[N],
                                          Sweep sweep)
    {
        static_assert(LEAN == 1 || LEAN == 2, "the packed loop has wh_march's LEAN forms only");
        pair_t p[N], q[N], hm[N], dm[N];
        const float half_dt = 0.5f * dt;
#pragma unroll
        for (int l = 0; l < N; ++l)
        {
            p[l] = q[l] = u[l] = v[l] = 0;
            hm[l] = half_dt * invm[l];
            dm[l] = ((DM >> l) & 1u) != 0 ? dt * invm[l] : pair_t{0.0f, 0.0f};
        }
        for (int whit = 0; whit < A.wh_iters; ++whit)
        {
            const float k0 = filt[0];
#pragma unroll
            for (int l = 0; l < N; ++l)
            {
                p[l] = u[l];
                q[l] = v[l];
                u[l] *= k0;
                v[l] *= k0;
            }
            for (int it = 1; it <= nt; ++it)
            {
                const float c0 = cs[2 * it - 2], s0 = sn[2 * it - 2];
                const float c1 = cs[2 * it - 1], s1 = sn[2 * it - 1];
                const float kw = filt[it];
                pair_t z[N], ph[N], qh[N];

                sweep(p, z);
#pragma unroll
                for (int l = 0; l < N; ++l)
                {
                    pair_t dq;
                    if (((INTERIOR >> l) & 1u) != 0)
                        dq = LEAN == 2 ? pk_fma(s0, Gf[l], pk_fma(c0, F[l], z[l])) : z[l];
                    else
                        dq = pk_fma(s0, Gf[l], pk_fma(c0, F[l], pk_fma(-Hi[l], q[l], z[l])));
                    ph[l] = pk_fma(-half_dt, q[l], p[l]);
                    qh[l] = pk_fma(hm[l], dq, q[l]);
                    p[l] = pk_fma(-dt, qh[l], p[l]);
                }
                sweep(ph, z);
#pragma unroll
                for (int l = 0; l < N; ++l)
                {
                    pair_t dq;
                    if (((INTERIOR >> l) & 1u) != 0)
                        dq = LEAN == 2 ? pk_fma(s1, Gf[l], pk_fma(c1, F[l], z[l])) : z[l];
                    else
                        dq = pk_fma(s1, Gf[l], pk_fma(c1, F[l], pk_fma(-Hi[l], qh[l], z[l])));
                    if (((DM >> l) & 1u) != 0)
                        q[l] = pk_fma(dm[l], dq, q[l]);
                    else
                        q[l] = pk_fma(hm[l], 2.0f * dq, q[l]);
                    u[l] = pk_fma(kw, p[l], u[l]);
                    v[l] = pk_fma(kw, q[l], v[l]);
                }
            }
        }
    }

    // Grids: nothing, or the plan's TimeGrids (kernel 13: a pass per distinct grid among the four rows, GroupedRows; RK2 only)
    // PAIRED: the paired chains in the sweep (element_lane_pair_product), the one-grid kernel only
    template <bool FORCED, bool HOLD, bool LAST_COPY, bool PAIRED, typename... Grids>
    __global__ void __launch_bounds__(256, 3) ddh_element_lane_kernel(DdhArgs<float> A, const float *__restrict__ Sep4, const float *__restrict__ filt,
                                                                     const float *__restrict__ cs, const float *__restrict__ sn, Grids... grids)
    {
        constexpr bool GROUPED = sizeof...(Grids) > 0;
        static_assert(sizeof...(Grids) <= 1 && scheme_of<Grids...> == 0, "one grid, or TimeGrids; no RK4 form");
        static_assert(!(PAIRED && sizeof...(Grids) > 0), "the paired chains are built for the one-grid kernel only");
        const int s_first = A.dom_begin + 4 * (blockIdx.x * 4 + (threadIdx.x >> 6));
        if (s_first >= A.dom_end)
            return; // wave-uniform: the kernel has no barriers
        if constexpr (HOLD)
            __builtin_amdgcn_s_setprio(3);
        [[maybe_unused]] const int w_first = wave_uniform(s_first); // GROUPED: the wavefront's first position, scalar
        [[maybe_unused]] int done = 0; // GROUPED: the rows that have published, a bit each; what a pass leaves to the next
        [[maybe_unused]] GroupedRows rows{}; // of the pass under way: locate forms it
        [[maybe_unused]] DdhArgs<float> Ap;  // GROUPED: A as the pass read it (reread_args)
        const DdhArgs<float> &Ar = [&]() -> const DdhArgs<float> &
        {
            if constexpr (GROUPED)
                return Ap;
            else
                return A;
        }();
        do
        {
        if constexpr (GROUPED)
            reread_args(Ap);
        // where this lane works: subdomain s (valid: and publishes it), its trace dofs, the dofs of its element's nodes
        auto locate = [&](int tid, bool &valid, int &s, int &fdof, const int *&sI)
        {
            const int sub = (tid >> 4) & 3;
            if constexpr (GROUPED)
            {
                // from the lane, w_first and done alone: behind the march nothing of the first time is there to be kept
                rows = grouped_rows(Ar, w_first, done, first_of(grids...));
                valid = grouped_row(Ar, w_first, sub, rows, first_of(grids...), s);
            }
            else
            {
                valid = s_first + sub < Ar.dom_end;
                s = domain_at(Ar, valid ? s_first + sub : s_first);
            }
            fdof = Ar.s_fdof[s];
            sI = Ar.sI + 256 * (size_t)s + 16 * (tid & 15);
        };
        bool valid;
        int s, fdof;
        const int *sI;
        int tid = threadIdx.x;
        if constexpr (GROUPED)
            tid = lane_here(); // a pass starts from a lane index of its own, or what the last pass derived from it waits through the march
        locate(tid, valid, s, fdof, sI);
        // 0, in a way the compiler cannot see (done < 16): W and 1 / W, which only the loads before the march need, are read
        // at an index that depends on the pass, or all of them are kept for the next pass, through the time loop
        [[maybe_unused]] const int again = GROUPED ? done >> 4 : 0;
        // the pass's time grid (the leader's; one grid: the launch's), scalar
        const TimeGridView<float> tg = time_grid_of(Ar, GROUPED ? rows.s_lead : s, filt, cs, sn, grids...);

        pair_t invm[8], Hi[8], F[8], Gf[8], u[8], v[8];
#pragma unroll
        for (int n = 0; n < 16; ++n)
        {
            const int P = el_pair(n & 3, n >> 2), half = el_half(n >> 2);
            float im, hi, f, gf;
            load_dof(Ar, s, sI[n], fdof, im, hi, f, gf);
            const float W = Sep4[48 + n + again], rW = Sep4[64 + n + again];
            invm[P][half] = im * W;
            Hi[P][half] = hi * rW;
            F[P][half] = f * rW;
            Gf[P][half] = gf * rW;
        }
        float By[16]; // wave-uniform: scalar registers for the whole time loop
        pair_t Bx[6], Dg[8];
#pragma unroll
        for (int i = 0; i < 16; ++i)
        {
            if ((i & 3) != (i >> 2))
                Bx[bx_slot(i & 3, i >> 2) / 2][bx_slot(i & 3, i >> 2) % 2] = Sep4[i]; // Bx(k, j) at k + 4 j, the off-diagonals
            By[i] = Sep4[16 + i]; // By(l, j) at l + 4 j
            Dg[el_pair(i & 3, i >> 2)][el_half(i >> 2)] = Sep4[32 + i]; // Dg(k, l) at k + 4 l
        }
        const float mR = (threadIdx.x & 3) < 3 ? 1.0f : 0.0f; // ex < 3: the only mask left, for the xi sums

        auto sweep = [&](const pair_t(&w)[8], pair_t(&z)[8])
        {
            element_lane_products_packed<PAIRED>(w, z, Bx, By, Dg);
            // xi neighbours: my k == 3 column meets the k == 0 column of lane + 1 (and vice versa); the 32-bit halves of the pairs
            float hi[4] = {z[3].x, z[7].x, z[7].y, z[3].y}, lo[4] = {z[0].x, z[4].x, z[4].y, z[0].y}; // l = 0, 1, 2, 3
            element_assemble_xi_row_asm(hi, lo, mR);
            z[3].x = hi[0], z[7].x = hi[1], z[7].y = hi[2], z[3].y = hi[3];
            z[0].x = lo[0], z[4].x = lo[1], z[4].y = lo[2], z[0].y = lo[3];
            // eta neighbours, on the xi-assembled values: my l == 3 row meets the l == 0 row of lane + 4
            float up[4] = {z[0].y, z[1].y, z[2].y, z[3].y}, dn[4] = {z[0].x, z[1].x, z[2].x, z[3].x};
            element_assemble_eta_row_asm(up, dn);
#pragma unroll
            for (int k = 0; k < 4; ++k)
            {
                z[k].y = up[k];
                z[k].x = dn[k];
            }
        };
        wh_march_pairs<FORCED ? 2 : 1, ELEMENT_INTERIOR_PAIRS, PAIRED ? ELEMENT_LANE_PAIRED_DM_PAIRS(FORCED) : ELEMENT_LANE_DM_PAIRS(FORCED)>(Ar, tg.nt, tg.dt, tg.filt, tg.cs, tg.sn, invm, Hi, F, Gf, u, v, sweep);

        // located a second time from a lane index the compiler cannot connect with the first: otherwise these values stay
        // in (or are spilled from) vector registers for the whole time loop, which runs at the limit of three wavefronts per SIMD
        if constexpr (GROUPED)
        {
            tid = lane_here();
            asm volatile("" : "+s"(done));
            reread_args(Ap);
        }
        else
        {
            tid = threadIdx.x;
            asm volatile("" : "+v"(tid));
        }
        locate(tid, valid, s, fdof, sI);
        if constexpr (!GROUPED)
            if (!valid)
                return;
#pragma unroll
        for (int n = 0; n < 16; ++n)
        {
            // every shared node is held by 2 or 4 (lane, register) pairs with identical values: the copy with
            // the smallest element-node index writes (with LAST_COPY the one with the largest)
            const int k = n & 3, l = n >> 2;
            const bool first = !(k == 0 && (tid & 3) > 0) && !(l == 0 && (tid & 12) > 0);
            const bool last = !(k == 3 && (tid & 3) < 3) && !(l == 3 && (tid & 12) < 12);
            const bool owner = (LAST_COPY ? last : first) && (!GROUPED || valid);
            if (owner)
                publish_dof(Ar, s, sI[n], fdof, u[el_pair(k, l)][el_half(l)], v[el_pair(k, l)][el_half(l)], false);
        }
        if constexpr (GROUPED)
            done |= grouped_published(rows, valid);
        } while (GROUPED && (rows.pending & ~done) != 0);
    }

    // ---------------------------------------------------------------- kernel 11 (NB = 4, 8x8 elements, rectangles): one subdomain per wavefront
    // The element-lane form with a subdomain of 64 elements: lane = element ex + 8 ey, register n = k + 4 l = node (k, l); the
    // tables, the in-lane products, the folded weight W and wh_march's LEAN rules are those of ddh_element_lane_kernel (the
    // element is the same rectangle whatever the subdomain).  Only the assembly differs.  xi neighbours are lane +- 1: a
    // 16-lane DPP row holds two eta-rows of elements, so the row shift by 1 also carries ex == 7 into the next eta-row's
    // ex == 0 (and back), which the masks mR / mL multiply by 0; past the ends of a DPP row bound_ctrl reads 0.  eta
    // neighbours are lane +- 8, half of them in another DPP row: ds_bpermute_b32 (the __shfl of ddh_mfma_kernel), 8 per sweep
    // on the LDS pipe, no LDS storage.  xi first, eta on the xi-assembled values, masks 0 / 1: the 2 or 4 copies of a shared
    // node form the same commutative sums and stay bitwise equal.  Four wavefronts per workgroup, no barriers.  A wavefront
    // holds one subdomain, so a launch of any length needs no padding rows and a subdomain's result does not depend on
    // which others the launch holds.
    // Compiled for three wavefronts per SIMD in the action form and two in the form with x.
    template <bool FORCED, bool HOLD, bool LAST_COPY, typename... Grids>
    __global__ void __launch_bounds__(256, FORCED ? 2 : 3) ddh_element_lane8_kernel(DdhArgs<float> A, const float *__restrict__ Sep4, const float *__restrict__ filt,
                                                                                   const float *__restrict__ cs, const float *__restrict__ sn, Grids... grids)
    {
        if (A.dom_begin + (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6) >= A.dom_end)
            return; // wave-uniform: the kernel has no barriers
        if constexpr (HOLD)
            __builtin_amdgcn_s_setprio(3);
        // with time grids the subdomain waits in one scalar register from here to the outputs: the list pointer that finding it
        // again would take has none left to wait in
        [[maybe_unused]] int s_wave = 0;
        if constexpr (sizeof...(Grids) > 0)
            s_wave = wave_uniform(domain_at(A, A.dom_begin + (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), grids...));
        // where this lane works: subdomain s, its trace dofs, the dofs of its element's nodes
        auto locate = [&](int tid, int &s, int &fdof, const int *&sI)
        {
            if constexpr (sizeof...(Grids) > 0)
                s = s_wave;
            else
                s = domain_at(A, A.dom_begin + (int)blockIdx.x * 4 + (tid >> 6));
            fdof = A.s_fdof[s];
            sI = A.sI + 1024 * (size_t)s + 16 * (tid & 63);
        };
        int s, fdof;
        const int *sI;
        locate(threadIdx.x, s, fdof, sI);
        // the time grid first, while few vector registers are live: what stays of it is scalar
        const TimeGridView<float> tg = time_grid_of(A, s, filt, cs, sn, grids...);
        const int lane = threadIdx.x & 63, ex = lane & 7, ey = lane >> 3;

        float invm[16], Hi[16], F[16], Gf[16], u[16], v[16];
#pragma unroll
        for (int n = 0; n < 16; ++n)
        {
            load_dof(A, s, sI[n], fdof, invm[n], Hi[n], F[n], Gf[n]);
            const float W = Sep4[48 + n], rW = Sep4[64 + n];
            invm[n] *= W;
            Hi[n] *= rW;
            F[n] *= rW;
            Gf[n] *= rW;
        }
        float Bx[16], By[16], Dg[16]; // wave-uniform: scalar registers for the whole time loop
#pragma unroll
        for (int i = 0; i < 16; ++i)
        {
            Bx[i] = Sep4[i];      // Bx(k, j) at k + 4 j
            By[i] = Sep4[16 + i]; // By(l, j) at l + 4 j
            Dg[i] = Sep4[32 + i]; // Dg(k, l) at k + 4 l
        }
        const float mR = ex < 7 ? 1.0f : 0.0f, mL = ex > 0 ? 1.0f : 0.0f, mU = ey < 7 ? 1.0f : 0.0f, mD = ey > 0 ? 1.0f : 0.0f;
        const int above = (lane + 8) & 63, below = (lane + 56) & 63; // a lane without that neighbour reads a lane it masks out

        auto sweep = [&](const float(&w)[16], float(&z)[16])
        {
            element_lane_products(w, z, Bx, By, Dg);
            // xi neighbours: my k == 3 column meets the k == 0 column of lane + 1 (and vice versa)
            float hi[4] = {z[3], z[7], z[11], z[15]}, lo[4] = {z[0], z[4], z[8], z[12]};
            element_assemble_xi_asm(hi, lo, mR, mL);
#pragma unroll
            for (int l = 0; l < 4; ++l)
            {
                z[3 + 4 * l] = hi[l];
                z[0 + 4 * l] = lo[l];
            }
            // eta neighbours, on the xi-assembled values: my l == 3 row meets the l == 0 row of lane + 8 (and vice versa)
#pragma unroll
            for (int k = 0; k < 4; ++k)
            {
                const float up = z[k + 12], dn = z[k];
                const float from_above = __shfl(dn, above, 64), from_below = __shfl(up, below, 64);
                z[k + 12] = up + mU * from_above;
                z[k] = dn + mD * from_below;
            }
        };
        wh_march<FORCED ? 2 : 1, ELEMENT_INTERIOR_REGISTERS>(A, tg.nt, tg.dt, tg.filt, tg.cs, tg.sn, invm, Hi, F, Gf, u, v, sweep);

        // located a second time from a lane index the compiler cannot connect with the first, as in ddh_element_lane_kernel
        // (with time grids the same for the subdomain in its scalar register: nothing derived from it waits through the loop)
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        if constexpr (sizeof...(Grids) > 0)
            asm volatile("" : "+s"(s_wave));
        locate(tid, s, fdof, sI);
#pragma unroll
        for (int n = 0; n < 16; ++n)
        {
            // every shared node is held by 2 or 4 (lane, register) pairs with identical values: the copy with
            // the smallest element-node index writes (with LAST_COPY the one with the largest)
            const int k = n & 3, l = n >> 2;
            const bool first = !(k == 0 && (tid & 7) > 0) && !(l == 0 && (tid & 56) > 0);
            const bool last = !(k == 3 && (tid & 7) < 7) && !(l == 3 && (tid & 56) < 56);
            const bool owner = LAST_COPY ? last : first;
            if (owner)
                publish_dof(A, s, sI[n], fdof, u[n], v[n], false);
        }
    }

    // ---------------------------------------------------------------- kernel 12 (NB = 5, 4x4 elements, rectangles): four subdomains per wavefront
    // ddh_element_lane_kernel's lane map with 25 nodes per lane: lane = element ex + 4 ey, one subdomain per 16-lane DPP row,
    // four subdomains per wavefront, register n = k + 5 l = node (k, l).  The sweep is the one documented there,
    //     z'(k,l) = Dg(k,l) w(k,l) + sum_{j != k} Bx(k,j) w(j,l) + sum_{j != l} By(l,j) w(k,j),   z = W z',
    // 9 in-lane FMAs per node with wave-uniform coefficients (20 + 20 + 25 scalars), W folded into the per-dof constants.
    // Assembly: the k == 4 column meets the k == 0 column of lane + 1, the l == 4 row the l == 0 row of lane + 4, five values
    // each, through the row forms above (one copy forms the sum, the other takes it; the shifts never leave the 16-lane row,
    // so a subdomain's result does not depend on its wave-mates); xi first, eta on the xi-assembled values.  The nine
    // registers with k, l in {1, 2, 3} are element-interior: wh_march's LEAN rules apply to them.  The time loop is wh_march,
    // node by node.  A launch whose length is no multiple of 4 recomputes the wavefront's first subdomain in the missing rows
    // and publishes nothing from them.  The action form is compiled for two wavefronts per SIMD (256 vector registers, no
    // scratch); the form with x (rhs, postprocess: once per solve) keeps the sources of the nine interior nodes as well and
    // takes one wavefront per SIMD, a few values in accumulation registers, no scratch either.  The 65 coefficients stay in
    // scalar registers through the time loop, which issues 736 vector instructions per wavefront-step in the action form
    // (774 with x), read from the code object; registers and scratch of every instantiation:
    // profiles/r19/ddh_nb5_registers.txt.
    constexpr unsigned ELEMENT5_INTERIOR_REGISTERS = (7u << 6) | (7u << 11) | (7u << 16);

    __device__ inline void element_lane5_products(const float (&w)[25], float (&z)[25], const float (&Bx)[25], const float (&By)[25],
                                                  const float (&Dg)[25])
    {
#pragma unroll
        for (int l = 0; l < 5; ++l)
#pragma unroll
            for (int k = 0; k < 5; ++k)
            {
                float t = Dg[k + 5 * l] * w[k + 5 * l];
#pragma unroll
                for (int j = 0; j < 5; ++j)
                {
                    if (j != k)
                        t += Bx[k + 5 * j] * w[j + 5 * l];
                    if (j != l)
                        t += By[l + 5 * j] * w[k + 5 * j];
                }
                z[k + 5 * l] = t;
            }
    }

    // Grids: nothing, or the plan's TimeGrids (kernel 13: a pass per distinct grid among the four rows, GroupedRows; RK2 only)
    template <bool FORCED, bool HOLD, bool LAST_COPY, typename... Grids>
    __global__ void __launch_bounds__(256, FORCED ? 1 : 2) ddh_element_lane5_kernel(DdhArgs<float> A, const float *__restrict__ Sep5, const float *__restrict__ filt,
                                                                      const float *__restrict__ cs, const float *__restrict__ sn, Grids... grids)
    {
        constexpr bool GROUPED = sizeof...(Grids) > 0;
        static_assert(sizeof...(Grids) <= 1 && scheme_of<Grids...> == 0, "one grid, or TimeGrids; no RK4 form");
        const int s_first = A.dom_begin + 4 * (blockIdx.x * 4 + (threadIdx.x >> 6));
        if (s_first >= A.dom_end)
            return; // wave-uniform: the kernel has no barriers
        if constexpr (HOLD)
            __builtin_amdgcn_s_setprio(3);
        [[maybe_unused]] const int w_first = wave_uniform(s_first); // GROUPED: the wavefront's first position, scalar
        [[maybe_unused]] int done = 0; // GROUPED: the rows that have published, a bit each; what a pass leaves to the next
        [[maybe_unused]] GroupedRows rows{}; // of the pass under way: locate forms it
        [[maybe_unused]] DdhArgs<float> Ap;  // GROUPED: A as the pass read it (reread_args)
        const DdhArgs<float> &Ar = [&]() -> const DdhArgs<float> &
        {
            if constexpr (GROUPED)
                return Ap;
            else
                return A;
        }();
        do
        {
        if constexpr (GROUPED)
            reread_args(Ap);
        // where this lane works: subdomain s (valid: and publishes it), its trace dofs, the dofs of its element's nodes
        auto locate = [&](int tid, bool &valid, int &s, int &fdof, const int *&sI)
        {
            const int sub = (tid >> 4) & 3;
            if constexpr (GROUPED)
            {
                // from the lane, w_first and done alone: behind the march nothing of the first time is there to be kept
                rows = grouped_rows(Ar, w_first, done, first_of(grids...));
                valid = grouped_row(Ar, w_first, sub, rows, first_of(grids...), s);
            }
            else
            {
                valid = s_first + sub < Ar.dom_end;
                s = domain_at(Ar, valid ? s_first + sub : s_first);
            }
            fdof = Ar.s_fdof[s];
            sI = Ar.sI + 400 * (size_t)s + 25 * (tid & 15);
        };
        bool valid;
        int s, fdof;
        const int *sI;
        int tid = threadIdx.x;
        if constexpr (GROUPED)
            tid = lane_here(); // a pass starts from a lane index of its own, or what the last pass derived from it waits through the march
        locate(tid, valid, s, fdof, sI);
        // 0, in a way the compiler cannot see (done < 16): W and 1 / W, which only the loads before the march need, are read
        // at an index that depends on the pass, or all of them are kept for the next pass, through the time loop
        [[maybe_unused]] const int again = GROUPED ? done >> 4 : 0;
        // the pass's time grid (the leader's; one grid: the launch's), scalar
        const TimeGridView<float> tg = time_grid_of(Ar, GROUPED ? rows.s_lead : s, filt, cs, sn, grids...);

        float invm[25], Hi[25], F[25], Gf[25], u[25], v[25];
#pragma unroll
        for (int n = 0; n < 25; ++n)
        {
            load_dof(Ar, s, sI[n], fdof, invm[n], Hi[n], F[n], Gf[n]);
            const float W = Sep5[75 + n + again], rW = Sep5[100 + n + again];
            invm[n] *= W;
            Hi[n] *= rW;
            F[n] *= rW;
            Gf[n] *= rW;
        }
        float Bx[25], By[25], Dg[25]; // wave-uniform
#pragma unroll
        for (int i = 0; i < 25; ++i)
        {
            Bx[i] = Sep5[i];      // Bx(k, j) at k + 5 j
            By[i] = Sep5[25 + i]; // By(l, j) at l + 5 j
            Dg[i] = Sep5[50 + i]; // Dg(k, l) at k + 5 l
        }
        const float mR = (threadIdx.x & 3) < 3 ? 1.0f : 0.0f; // ex < 3: the only mask, for the xi sums

        auto sweep = [&](const float(&w)[25], float(&z)[25])
        {
            element_lane5_products(w, z, Bx, By, Dg);
            // xi neighbours: my k == 4 column meets the k == 0 column of lane + 1 (and vice versa)
            float hi[5] = {z[4], z[9], z[14], z[19], z[24]}, lo[5] = {z[0], z[5], z[10], z[15], z[20]};
            element_assemble_xi_row5_asm(hi, lo, mR);
#pragma unroll
            for (int l = 0; l < 5; ++l)
            {
                z[4 + 5 * l] = hi[l];
                z[0 + 5 * l] = lo[l];
            }
            // eta neighbours, on the xi-assembled values: my l == 4 row meets the l == 0 row of lane + 4
            float up[5] = {z[20], z[21], z[22], z[23], z[24]}, dn[5] = {z[0], z[1], z[2], z[3], z[4]};
            element_assemble_eta_row5_asm(up, dn);
#pragma unroll
            for (int k = 0; k < 5; ++k)
            {
                z[k + 20] = up[k];
                z[k] = dn[k];
            }
        };
        wh_march<FORCED ? 2 : 1, ELEMENT5_INTERIOR_REGISTERS>(Ar, tg.nt, tg.dt, tg.filt, tg.cs, tg.sn, invm, Hi, F, Gf, u, v, sweep);

        // located a second time from a lane index the compiler cannot connect with the first, as in ddh_element_lane_kernel
        if constexpr (GROUPED)
        {
            tid = lane_here();
            asm volatile("" : "+s"(done));
            reread_args(Ap);
        }
        else
        {
            tid = threadIdx.x;
            asm volatile("" : "+v"(tid));
        }
        locate(tid, valid, s, fdof, sI);
        if constexpr (!GROUPED)
            if (!valid)
                return;
#pragma unroll
        for (int n = 0; n < 25; ++n)
        {
            // every shared node is held by 2 or 4 (lane, register) pairs with identical values: the copy with
            // the smallest element-node index writes (with LAST_COPY the one with the largest)
            const int k = n % 5, l = n / 5;
            const bool first = !(k == 0 && (tid & 3) > 0) && !(l == 0 && (tid & 12) > 0);
            const bool last = !(k == 4 && (tid & 3) < 3) && !(l == 4 && (tid & 12) < 12);
            const bool owner = (LAST_COPY ? last : first) && (!GROUPED || valid);
            if (owner)
                publish_dof(Ar, s, sI[n], fdof, u[n], v[n], false);
        }
        if constexpr (GROUPED)
            done |= grouped_published(rows, valid);
        } while (GROUPED && (rows.pending & ~done) != 0);
    }

    // kernels 5, 8, 11 and 12 leave the boundary terms out on the element-interior nodes (k, l in 1 .. nb - 2): is none of them a
    // trace dof (sI >= s_fdof) in any subdomain?  True for every plan built from blocks of elements, where trace dofs lie on the
    // subdomain's boundary; a descriptor from elsewhere is checked, not trusted.
    // n_elems (16 or 64) elements of nb x nb nodes per subdomain, `stride` = nb nb n_elems entries of sI per subdomain.
    __global__ void __launch_bounds__(256) ddh_interior_check_kernel(int n_domains, int nb, int n_elems, int stride, const int *__restrict__ s_fdof,
                                                                     const int *__restrict__ sI, int *__restrict__ bad)
    {
        const int s = blockIdx.x, inner = nb - 2;
        if (s >= n_domains)
            return;
        for (int t = threadIdx.x; t < inner * inner * n_elems; t += 256)
        {
            const int i = t / n_elems, node = (1 + i % inner) + nb * (1 + i / inner) + nb * nb * (t % n_elems);
            if (sI[node + stride * (size_t)s] < s_fdof[s])
                atomicExch(bad, 1);
        }
    }

    // is the metric tensor of every element of every subdomain identical to that of (subdomain 0, element 0)?  (compared in the
    // plan's precision: float for kernel 5, double for kernel 8)
    template <typename Real>
    __global__ void __launch_bounds__(256) ddh_uniform_check_kernel(long long n_nodes_total, int nodes_per_elem, const Real *__restrict__ G,
                                                                    int *__restrict__ bad)
    {
        for (long long t = blockIdx.x * 256LL + threadIdx.x; t < n_nodes_total; t += gridDim.x * 256LL)
        {
            const int node = static_cast<int>(t % nodes_per_elem); // node within its element
            const Real *g = G + 3 * t, *g0 = G + 3 * node;
            if (g[0] != g0[0] || g[1] != g0[1] || g[2] != g0[2])
                atomicExch(bad, 1);
        }
    }

    // structure check for the wave kernels (NB nodes per direction, NEL x NEL elements in the order ex + NEL ey, at most 1024
    // element nodes): the expected number of dofs, and xi/eta neighbours share exactly the expected nodes
    template <int NB, int NEL>
    __global__ void __launch_bounds__(256) ddh_wave_check_kernel(int n_domains, const int *__restrict__ s_dof, const int *__restrict__ sI,
                                                                 int *__restrict__ bad)
    {
        constexpr int SIDE = NB * NEL - (NEL - 1), NDOF = SIDE * SIDE, NN = NB * NB, NODES = NN * NEL * NEL;
        const int s = blockIdx.x;
        if (s >= n_domains)
            return;
        const int *I = sI + NODES * (size_t)s;
        bool ok = true;
        for (int node = threadIdx.x; node < NODES; node += 256)
        {
            const int k = node % NB, l = (node / NB) % NB, el = node / NN, ex = el % NEL, ey = el / NEL;
            ok = ok && I[node] >= 0 && I[node] < NDOF;
            if (node == 0)
                ok = ok && s_dof[s] == NDOF;
            if (k == NB - 1 && ex < NEL - 1)
                ok = ok && I[node] == I[0 + NB * (l + NB * (el + 1))];
            if (l == NB - 1 && ey < NEL - 1)
                ok = ok && I[node] == I[k + NB * (0 + NB * (el + NEL))];
        }
        if (!ok)
            atomicExch(bad, 1);
    }

    // ---------------------------------------------------------------- workgroup-per-subdomain kernel (generic)
    // CSR = true is kernel 10: the contributor lists come from the plan (any valence) instead of being built with atomics.
    // MAXT: the launch bound, 256 or, for subdomains of 257 to 1024 element nodes, 1024 (at most 128 vector registers then).
    template <typename Real, int NB, bool CSR = false, int MAXT = 256, typename... Grids>
    __global__ void __launch_bounds__(MAXT) ddh_block_kernel(DdhArgs<Real> A, const Real *__restrict__ Dmat, const Real *__restrict__ filt,
                                                           const Real *__restrict__ cs, const Real *__restrict__ sn, Grids... grids)
    {
        raise_priority(A.prio);
        const int T = A.nodes; // == blockDim.x
        const int tid = threadIdx.x;
        const int s = domain_at(A, A.dom_begin + blockIdx.x, grids...);

        extern __shared__ double lds_raw[];
        Real *s_p = reinterpret_cast<Real *>(lds_raw); // [T] field, indexed by subdomain dof
        Real *s_f1 = s_p + T;                           // [T] fluxes, indexed by element node
        Real *s_f2 = s_f1 + T;
        Real *s_su = s_f2 + T;                          // [T] element contributions
        int *s_cnt = reinterpret_cast<int *>(s_su + T); // [T]
        int *s_lst = s_cnt + T;                         // [T][4]

        const int ndof = A.s_dof[s], fdof = A.s_fdof[s];
        const int k = tid % NB, l = (tid / NB) % NB, el = tid / (NB * NB);
        const int *sI = A.sI + (size_t)T * s;
        const int mydof = sI[tid];
        const bool active = mydof >= 0;

        int row[NB], col[NB];
        Real Dk[NB], Dl[NB], DTk[NB], DTl[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i)
        {
            row[i] = active ? sI[i + NB * (l + NB * el)] : 0; // dof of node (i, l)
            col[i] = active ? sI[k + NB * (i + NB * el)] : 0; // dof of node (k, i)
            Dk[i] = Dmat[k + NB * i];
            Dl[i] = Dmat[l + NB * i];
            DTk[i] = Dmat[i + NB * k];
            DTl[i] = Dmat[i + NB * l];
        }
        const Real *g = A.G + 3 * ((size_t)tid + (size_t)T * s);
        const Real g0 = active ? g[0] : Real(0), g1 = active ? g[1] : Real(0), g2 = active ? g[2] : Real(0);

        // who contributes to dof `tid`: element nodes in increasing order (fixed summation order)
        int nc = 0, c[4] = {0, 0, 0, 0};
        int c_first = 0; // CSR: my list is s_lst[c_first, c_first + nc)
        if constexpr (CSR)
        {
            const int *off = A.csr_off + (size_t)(T + 1) * s;
            if (tid < off[ndof])
                s_lst[tid] = A.csr_src[(size_t)T * s + tid];
            if (tid < ndof)
            {
                c_first = off[tid];
                nc = off[tid + 1] - c_first;
            }
        }
        else
        {
            s_cnt[tid] = 0;
            __syncthreads();
            if (active)
            {
                const int slot = atomicAdd(&s_cnt[mydof], 1);
                if (slot < 4)
                    s_lst[4 * mydof + slot] = tid;
            }
            __syncthreads();
            if (tid < ndof)
            {
                nc = s_cnt[tid];
                if (nc > 4)
                    __builtin_trap(); // more than four elements meet at a node: not a structured subdomain
                for (int j = 0; j < nc; ++j)
                    c[j] = s_lst[4 * tid + j];
                for (int a = 1; a < nc; ++a) // insertion sort of at most 4 entries
                    for (int b = a; b > 0 && c[b - 1] > c[b]; --b)
                    {
                        const int t = c[b];
                        c[b] = c[b - 1];
                        c[b - 1] = t;
                    }
            }
        }

        // per-dof data
        int g_idx = -1;
        Real ai = 0, mi = 0, inv_mi = 0, Hi = 0, F = 0, G = 0, lam = 0, mu = 0;
        Real u = 0, v = 0, p = 0, q = 0;
        const size_t dbase = (size_t)A.mx_dof * s, fbase = (size_t)A.mx_fdof * s;
        if (tid < ndof)
        {
            g_idx = A.gI[dbase + tid];
            ai = A.a[dbase + tid];
            mi = A.m[dbase + tid];
            inv_mi = Real(1) / (ai * ai * mi);
            if (A.x)
            {
                F = static_cast<Real>(A.x[g_idx]);
                G = static_cast<Real>(A.x[A.g_ndof + g_idx]);
            }
        }
        if (tid < fdof)
        {
            Hi = A.H[fbase + tid];
            if (A.lambda)
            {
                const int slot = A.B[tid + (size_t)A.mx_fdof * (0 + 2 * (size_t)s)];
                if (slot >= 0)
                {
                    lam = A.lambda[slot];
                    mu = A.lambda[A.n_lambda + slot];
                    F += Hi * lam;
                    G += Hi * mu;
                }
            }
            Hi *= ai;
        }

        // one stiffness sweep: field in s_p (already published), returns (S field)[tid] for tid < ndof
        auto sweep = [&]() -> Real
        {
            Real Ux = 0, Uy = 0;
#pragma unroll
            for (int i = 0; i < NB; ++i)
            {
                Ux += Dk[i] * s_p[row[i]];
                Uy += Dl[i] * s_p[col[i]];
            }
            s_f1[tid] = g0 * Ux + g1 * Uy;
            s_f2[tid] = g1 * Ux + g2 * Uy;
            __syncthreads();
            Real Su = 0;
#pragma unroll
            for (int i = 0; i < NB; ++i)
            {
                Su += DTk[i] * s_f1[i + NB * (l + NB * el)];
                Su += DTl[i] * s_f2[k + NB * (i + NB * el)];
            }
            s_su[tid] = Su;
            __syncthreads();
            Real z = 0;
            if constexpr (CSR)
                for (int j = 0; j < nc; ++j)
                    z += s_su[s_lst[c_first + j]];
            else
                for (int j = 0; j < nc; ++j)
                    z += s_su[c[j]];
            return z;
        };

        const TimeGridView<Real> tg = time_grid_of(A, s, filt, cs, sn, grids...);
        if constexpr (scheme_of<Grids...> == 1)
        {
            // RK4: wh_march on the thread's one value.  The sweep publishes the stage's field and is a workgroup phase like the
            // loop below: every thread of the workgroup marches the same subdomain, so all run the same number of sweeps
            const Real invm1[1] = {inv_mi}, Hi1[1] = {Hi}, F1[1] = {F}, G1[1] = {G};
            Real u1[1], v1[1];
            wh_march<0, 1u, 1>(A, tg.nt, tg.dt, tg.filt, tg.cs, tg.sn, invm1, Hi1, F1, G1, u1, v1, [&](const Real(&w)[1], Real(&z)[1])
                               {
                                   s_p[tid] = w[0];
                                   __syncthreads();
                                   z[0] = sweep();
                               });
            u = u1[0];
            v = v1[0];
        }
        else
        {
        const Real dt = tg.dt, half_dt = Real(0.5) * tg.dt;
        const int nt = tg.nt;
        for (int whit = 0; whit < A.wh_iters; ++whit)
        {
            const Real k0 = tg.filt[0];
            p = u;
            q = v;
            u *= k0;
            v *= k0;
            for (int it = 1; it <= nt; ++it)
            {
                s_p[tid] = p;
                __syncthreads();
                Real z = sweep() - Hi * q;
                Real dq = (z + tg.cs[2 * it - 2] * F + tg.sn[2 * it - 2] * G) * inv_mi;
                const Real ph = p - half_dt * q;
                const Real qh = q + half_dt * dq;
                p -= dt * qh;

                s_p[tid] = ph;
                __syncthreads();
                z = sweep() - Hi * qh;
                dq = (z + tg.cs[2 * it - 1] * F + tg.sn[2 * it - 1] * G) * inv_mi;
                q += dt * dq;

                const Real kw = tg.filt[it];
                u += kw * p;
                v += kw * q;
            }
        }
        }

        v *= Real(1) / A.omega;

        if (A.y && tid < ndof)
        {
            const Real M = mi * A.gmi[dbase + tid];
            if (CSR && A.unique_y)
            {
                A.y[g_idx] += static_cast<double>(M * u);
                A.y[A.g_ndof + g_idx] += static_cast<double>(M * v);
            }
            else
            {
                atomic_add(A.y + g_idx, static_cast<double>(M * u));
                atomic_add(A.y + A.g_ndof + g_idx, static_cast<double>(M * v));
            }
        }
        if (A.update && tid < fdof)
        {
            const int wslot = A.B[tid + (size_t)A.mx_fdof * (1 + 2 * (size_t)s)];
            if (wslot >= 0)
            {
                const Real S = Real(2) * ai * A.omega;
                A.update[wslot] = -lam - S * v;
                A.update[A.n_lambda + wslot] = -mu + S * u;
            }
        }
    }

    // ---------------------------------------------------------------- geometric factors (K13)
    template <typename Real>
    __global__ void __launch_bounds__(256) ddh_geom_kernel(long long total, int nodes, int nb, int mx_elems, const int *__restrict__ n_elems,
                                                          const int *__restrict__ elems, const double *__restrict__ w,
                                                          const double *__restrict__ J, const double *__restrict__ corners,
                                                          const double *__restrict__ pts, Real *__restrict__ G)
    {
        for (long long t = blockIdx.x * 256LL + threadIdx.x; t < total; t += gridDim.x * 256LL)
        {
            const int s = static_cast<int>(t / nodes), node = static_cast<int>(t % nodes);
            const int i = node % nb, j = (node / nb) % nb, el = node / (nb * nb);
            Real *g = G + 3 * t;
            if (el >= n_elems[s])
            {
                g[0] = g[1] = g[2] = 0;
                continue;
            }
            const int g_el = elems[el + (size_t)mx_elems * s];
            const double W = w[i] * w[j];
            double j4[4];
            if (J)
            {
                const double *Jp = J + 4 * ((size_t)i + nb * ((size_t)j + nb * (size_t)g_el));
                j4[0] = Jp[0], j4[1] = Jp[1], j4[2] = Jp[2], j4[3] = Jp[3];
            }
            else // straight from the element's corners: no (2, 2, nb, nb, g_elem) table
                bilinear_jacobian(corners + 8 * (size_t)g_el, pts[i], pts[j], j4);
            const double x_xi = j4[0], y_xi = j4[1], x_eta = j4[2], y_eta = j4[3];
            const double det = x_xi * y_eta - x_eta * y_xi;
            g[0] = static_cast<Real>(W * (y_eta * y_eta + x_eta * x_eta) / det);
            g[1] = static_cast<Real>(-W * (y_xi * y_eta + x_xi * x_eta) / det);
            g[2] = static_cast<Real>(W * (y_xi * y_xi + x_xi * x_xi) / det);
        }
    }

    template <typename Real>
    int geom_setup(int n_domains, int mx_elems, int nb, const int *n_elems, const int *elems, const double *w, const double *J,
                   const double *corners, const double *pts, Real *G, void *stream)
    {
        const int nodes = nb * nb * mx_elems;
        const long long total = (long long)nodes * n_domains;
        if (total <= 0)
            return 0;
        hipLaunchKernelGGL((ddh_geom_kernel<Real>), dim3(stream_grid(total, 256)), dim3(256), 0, as_stream(stream), total, nodes, nb,
                           mx_elems, n_elems, elems, w, J, corners, pts, G);
        return launch_status();
    }

    // Runs a check kernel that raises a device flag on the first violation it finds (launch(flag) starts it on the null
    // stream).  *bad = the flag, 1 if anything failed.  Returns a HIP error code.
    template <typename Launch>
    int device_flag_check(int *bad, Launch launch)
    {
        *bad = 1;
        int *flag = nullptr;
        hipError_t e = hipMalloc(&flag, sizeof(int));
        if (e == hipSuccess)
            e = hipMemset(flag, 0, sizeof(int));
        if (e == hipSuccess)
        {
            launch(flag);
            e = hipMemcpy(bad, flag, sizeof(int), hipMemcpyDeviceToHost);
        }
        if (flag)
            (void)hipFree(flag);
        return static_cast<int>(e);
    }

    // Does every element of every subdomain have the metric tensor of (subdomain 0, element 0)?  0 if so, -1 if not, > 0 on a
    // HIP error.
    template <typename Real>
    int check_uniform_geometry(const cuddh_ddh_desc &d, int nodes_per_elem, int nodes = 256)
    {
        const long long n_nodes = static_cast<long long>(nodes) * d.n_domains;
        int bad = 1;
        const int e = device_flag_check(&bad, [&](int *flag)
                                        { hipLaunchKernelGGL(ddh_uniform_check_kernel<Real>, dim3(stream_grid(n_nodes, 256)), dim3(256), 0, nullptr,
                                                             n_nodes, nodes_per_elem, static_cast<const Real *>(d.G), flag); });
        return e ? e : (bad ? -1 : 0);
    }

    // Builds plan->Aop for kernel 5 (Real = float) or plan->Aop64 for kernel 8 (Real = double), after establish_facts has
    // found one metric for all elements and no trace dof on an element-interior node.  Returns 0 or a HIP error.
    template <typename Real>
    int build_dense_element_matrix(cuddh_ddh_plan *p)
    {
        const cuddh_ddh_desc &d = p->d;
        Real hD[16], hG[48];
        hipError_t e = hipMemcpy(hD, d.D, sizeof hD, hipMemcpyDeviceToHost);
        if (e == hipSuccess)
            e = hipMemcpy(hG, d.G, sizeof hG, hipMemcpyDeviceToHost);
        if (e != hipSuccess)
            return static_cast<int>(e);

        // K[n_out][n_in], n = k + 4 l: one stiffness sweep (source/DDH.cpp:60-109) applied to unit vectors, in double
        auto Dm = [&](int a, int b) { return static_cast<double>(hD[a + 4 * b]); }; // D(a,b)
        double K[16][16];
        for (int nin = 0; nin < 16; ++nin)
        {
            double U[16] = {0};
            U[nin] = 1.0;
            double f1[16], f2[16];
            for (int l = 0; l < 4; ++l)
                for (int k = 0; k < 4; ++k)
                {
                    double ux = 0, uy = 0;
                    for (int i = 0; i < 4; ++i)
                    {
                        ux += Dm(k, i) * U[i + 4 * l];
                        uy += Dm(l, i) * U[k + 4 * i];
                    }
                    const Real *g = hG + 3 * (k + 4 * l);
                    f1[k + 4 * l] = g[0] * ux + g[1] * uy;
                    f2[k + 4 * l] = g[1] * ux + g[2] * uy;
                }
            for (int l = 0; l < 4; ++l)
                for (int k = 0; k < 4; ++k)
                {
                    double su = 0;
                    for (int i = 0; i < 4; ++i)
                        su += Dm(i, k) * f1[i + 4 * l] + Dm(i, l) * f2[k + 4 * i];
                    K[k + 4 * l][nin] = su;
                }
        }
        // A operand of step st, lane ln:  A[i = ln & 15][kk = 4 st + (ln >> 4)] = K'[m = i][nu = kk].  Columns: nu = 4 r_in + g_in
        // is node_of(g_in, r_in).  Rows follow the C/D map: m = 4 g_out + r_out for v_mfma_f32_16x16x4_f32
        // (row = 4 (lane >> 4) + reg), m = g_out + 4 r_out for v_mfma_f64_16x16x4_f64 (row = (lane >> 4) + 4 reg); either way
        // lane (el, g) gets node_of(g, r) in register r.
        constexpr bool F64 = sizeof(Real) == 8;
        Real hA[256];
        for (int st = 0; st < 4; ++st)
            for (int ln = 0; ln < 64; ++ln)
            {
                const int m = ln & 15, nu = 4 * st + (ln >> 4);
                const int g_out = F64 ? (m & 3) : (m >> 2), r_out = F64 ? (m >> 2) : (m & 3), r_in = nu >> 2, g_in = nu & 3;
                hA[64 * st + ln] = static_cast<Real>(K[node_of(g_out, r_out)][node_of(g_in, r_in)]);
            }
        Real *dA = nullptr;
        e = hipMalloc(reinterpret_cast<void **>(&dA), sizeof hA);
        if (e == hipSuccess)
            e = hipMemcpy(dA, hA, sizeof hA, hipMemcpyHostToDevice);
        if constexpr (F64)
            p->Aop64 = dA;
        else
            p->Aop = dA;
        return static_cast<int>(e);
    }

    // D and the metric tensor of element 0 on the host, for the tables of the separable sweeps (element_lane_tables.hpp: kernel 7,
    // NB = 8; the element-lane kernels, NB = 4 and 5).  The caller has found element 0's metric to be that of all elements
    // (check_uniform_geometry).  Returns 0 or a HIP error.
    template <int NB>
    int download_element(const cuddh_ddh_desc &d, float (&hD)[NB * NB], float (&hG)[3 * NB * NB])
    {
        hipError_t e = hipMemcpy(hD, d.D, sizeof hD, hipMemcpyDeviceToHost);
        if (e == hipSuccess)
            e = hipMemcpy(hG, d.G, sizeof hG, hipMemcpyDeviceToHost);
        return static_cast<int>(e);
    }

    template <size_t N>
    int upload_table(float **dst, const float (&h)[N])
    {
        hipError_t e = hipMalloc(reinterpret_cast<void **>(dst), sizeof h);
        if (e == hipSuccess)
            e = hipMemcpy(*dst, h, sizeof h, hipMemcpyHostToDevice);
        return static_cast<int>(e);
    }

    // kernel 7 tables.  Returns 0 on success, -1 when the geometry does not qualify, > 0 on a HIP error.
    int build_separable_tables(cuddh_ddh_plan *p)
    {
        double Ax[8][8], Ay[8][8], beta[8], gamma[8];
        float hD[64], hG[192];
        if (const int c = download_element<8>(p->d, hD, hG))
            return c;
        if (const int c = separable_factors<8>(hD, hG, Ax, Ay, beta, gamma))
            return c;
        float hS[144] = {0};
        for (int a = 0; a < 8; ++a)
            for (int b = 0; b < 8; ++b)
            {
                hS[a + 8 * b] = static_cast<float>(Ax[a][b]);
                if (a <= b)
                    hS[64 + sym_index(a, b)] = static_cast<float>(Ay[a][b]); // Ay(a,b) == Ay(b,a)
            }
        for (int i = 0; i < 8; ++i)
        {
            hS[128 + i] = static_cast<float>(beta[i]);
            hS[136 + i] = static_cast<float>(gamma[i]);
        }
        return upload_table(&p->Sep, hS);
    }

    // Tables of the element-lane kernels: kernel 5's element-lane form and kernel 11 (NB = 4), kernel 12 (NB = 5).  The
    // arithmetic and the checks are host code (element_lane_tables.hpp: separable metric, node weight W positive and the same
    // on both sides of every shared edge; all elements are identical, so that covers every copy of every shared dof).
    // Sep4 = [Bx(k,j) at k + NB j | By(l,j) at l + NB j | Dg(k,l) at k + NB l | W | 1 / W], NB^2 floats each.  Returns 0 on success,
    // -1 when the geometry does not qualify (p->Sep4 stays null: a kernel-5 plan stays on the matrix form), > 0 on a HIP error.
    // Called after the caller has checked that all elements share one metric.
    template <int NB>
    int build_element_lane_tables(cuddh_ddh_plan *p)
    {
        float hD[NB * NB], hG[3 * NB * NB], hS[5 * NB * NB];
        if (const int c = download_element<NB>(p->d, hD, hG))
            return c;
        if (const int c = element_lane_tables<NB>(hD, hG, hS))
            return c;
        return upload_table(&p->Sep4, hS);
    }

    // ---------------------------------------------------------------- what plan creation establishes about the descriptor
    // Runs the checks and table builders ddh_checks() lists for the plan's shape and request, in that order (four bits each,
    // the first in the lowest), up to the first that does not hold, and sets the bit of each that held in p->facts.  A plan
    // thus runs the device checks of the kernels it may take and no others.  Returns 0 or a HIP error.
    template <typename Real, int NB, int NEL>
    int establish_facts(cuddh_ddh_plan *p, unsigned checks)
    {
        constexpr int NN = NB * NB, ELEMS = NEL * NEL, NODES = NN * ELEMS;
        const cuddh_ddh_desc &d = p->d;
        for (; checks != 0; checks >>= 4)
        {
            int held = -1, bad = 1; // held: 0 yes, -1 no, > 0 a HIP error
            switch (checks & 15)
            {
            case DDH_STRUCTURE: // the NEL x NEL element layout the wavefront kernels assume
                held = device_flag_check(&bad, [&](int *flag)
                                         { hipLaunchKernelGGL((ddh_wave_check_kernel<NB, NEL>), dim3(d.n_domains), dim3(256), 0, nullptr, d.n_domains,
                                                              d.s_dof, d.sI, flag); });
                held = held ? held : -bad;
                break;
            case DDH_UNIFORM: held = check_uniform_geometry<Real>(d, NN, NODES); break;
            case DDH_INTERIOR:
                held = device_flag_check(&bad, [&](int *flag)
                                         { hipLaunchKernelGGL(ddh_interior_check_kernel, dim3(d.n_domains), dim3(256), 0, nullptr, d.n_domains, NB,
                                                              ELEMS, NODES, d.s_fdof, d.sI, flag); });
                held = held ? held : -bad;
                break;
            case DDH_DENSE:
                if constexpr (NB == 4 && NEL == 4)
                    held = build_dense_element_matrix<Real>(p);
                break;
            case DDH_SEP8:
                if constexpr (NB == 8)
                    held = build_separable_tables(p);
                break;
            case DDH_LANE:
                if constexpr (NB == 4 || NB == 5)
                    held = build_element_lane_tables<NB>(p);
                break;
            }
            if (held > 0)
                return held;
            if (held < 0)
                break;
            p->facts |= ddh_fact(checks & 15);
        }
        return 0;
    }

    // the shapes with checks of their own (ddh_checks lists none for any other)
    template <typename Real>
    int establish_facts(cuddh_ddh_plan *p, unsigned checks)
    {
        const int nb = p->d.nb, nel = p->d.nel1d;
        if (nb == 4 && nel == 4)
            return establish_facts<Real, 4, 4>(p, checks);
        if (nb == 8 && nel == 2)
            return establish_facts<Real, 8, 2>(p, checks);
        if (nb == 4 && nel == 8)
            return establish_facts<Real, 4, 8>(p, checks);
        if (nb == 5 && nel == 4)
            return establish_facts<Real, 5, 4>(p, checks);
        return checks == 0 ? 0 : static_cast<int>(hipErrorInvalidValue);
    }

    // ---------------------------------------------------------------- launches
    // (runtime flags become template arguments in with_flags, common.hpp, and nowhere else)

    // n_basis becomes a template argument here: the orders kernels 1 and 10 are built for are listed here and nowhere else
    template <class F>
    void with_n_basis(int nb, F &&f)
    {
        using std::integral_constant;
        switch (nb)
        {
        case 2: return f(integral_constant<int, 2>{});
        case 3: return f(integral_constant<int, 3>{});
        case 4: return f(integral_constant<int, 4>{});
        case 5: return f(integral_constant<int, 5>{});
        case 6: return f(integral_constant<int, 6>{});
        case 7: return f(integral_constant<int, 7>{});
        case 8: return f(integral_constant<int, 8>{});
        case 9: return f(integral_constant<int, 9>{});
        case 10: return f(integral_constant<int, 10>{});
        }
    }

    // The time tables and the trailing arguments of a plan's launches: f(filter, cs, sn, options...).  One time grid: the
    // descriptor's tables and nothing; GRIDS: the plan's concatenated per-grid tables and its TimeGrids; RK4: the scheme's tag
    // comes last.  The kernels are instantiated with the types of `options` as their trailing pack.
    template <typename Real, bool GRIDS, bool RK4, class F>
    void with_tables(const cuddh_ddh_plan *p, F &&f)
    {
        auto typed = [&](const void *fl, const void *cs, const void *sn, auto... options)
        {
            if constexpr (RK4)
                f(static_cast<const Real *>(fl), static_cast<const Real *>(cs), static_cast<const Real *>(sn), options..., Rk4Scheme{});
            else
                f(static_cast<const Real *>(fl), static_cast<const Real *>(cs), static_cast<const Real *>(sn), options...);
        };
        if constexpr (GRIDS)
            typed(p->grid_filter, p->grid_cs, p->grid_sn, TimeGrids<Real>{p->grid_of, static_cast<const DdhTimeGrid<Real> *>(p->grids)});
        else
            typed(p->d.wh_filter, p->d.cs, p->d.sn);
    }

    dim3 launch_grid(const cuddh_ddh_plan *p, int n_local) { return dim3((n_local + p->launch.per_group - 1) / p->launch.per_group); }

    // The plan kernels: each is launched from exactly one place, with the geometry resolve() stored.  What belongs to the call
    // and not to the plan, sources or none (A.x) and the priority, is branched on here.
    template <typename Real, int NB, bool CSR, int MAXT, bool GRIDS, bool RK4>
    void run_block(const cuddh_ddh_plan *p, const DdhArgs<Real> &A, int n_local, hipStream_t st) // kernels 1 and 10
    {
        with_tables<Real, GRIDS, RK4>(p, [&](const Real *fl, const Real *cs, const Real *sn, auto... o)
                                      { hipLaunchKernelGGL((ddh_block_kernel<Real, NB, CSR, MAXT, decltype(o)...>), launch_grid(p, n_local),
                                                           dim3(p->launch.block), p->launch.lds, st, A, static_cast<const Real *>(p->d.D), fl, cs, sn, o...); });
    }

    template <typename Real, int VAR, bool GRIDS, bool RK4>
    void run_wave(const cuddh_ddh_plan *p, const DdhArgs<Real> &A, int n_local, hipStream_t st) // kernels 2, 3 and 4
    {
        with_tables<Real, GRIDS, RK4>(p, [&](const Real *fl, const Real *cs, const Real *sn, auto... o)
                                      { hipLaunchKernelGGL((ddh_wave_kernel<Real, VAR, decltype(o)...>), launch_grid(p, n_local), dim3(p->launch.block), 0,
                                                           st, A, static_cast<const Real *>(p->d.D), fl, cs, sn, o...); });
    }

    template <typename Real, int VAR, bool GRIDS, bool RK4>
    void run_general_wave(const cuddh_ddh_plan *p, const DdhArgs<Real> &A, int n_local, hipStream_t st) // kernel 9
    {
        with_tables<Real, GRIDS, RK4>(p, [&](const Real *fl, const Real *cs, const Real *sn, auto... o)
                                      { hipLaunchKernelGGL((ddh_general_wave_kernel<Real, VAR, decltype(o)...>), launch_grid(p, n_local),
                                                           dim3(p->launch.block), 0, st, A, static_cast<const Real *>(p->d.D), fl, cs, sn, o...); });
    }

    template <typename Real, bool ASM, bool SEP>
    void run_wave8(const cuddh_ddh_plan *p, const DdhArgs<Real> &A, int n_local, hipStream_t st) // kernels 6 and 7: one grid, RK2
    {
        with_tables<Real, false, false>(p, [&](const Real *fl, const Real *cs, const Real *sn)
                                        { hipLaunchKernelGGL((ddh_wave8_kernel<Real, ASM, SEP>), launch_grid(p, n_local), dim3(p->launch.block), 0, st, A,
                                                             static_cast<const Real *>(p->d.D), fl, cs, sn, reinterpret_cast<const Real *>(p->Sep)); });
    }

    template <typename Real, bool GRIDS, bool RK4>
    void run_mfma(const cuddh_ddh_plan *p, const DdhArgs<Real> &A, int n_local, hipStream_t st) // kernel 5 (matrix form) and 8
    {
        const Real *K = sizeof(Real) == 4 ? reinterpret_cast<const Real *>(p->Aop) : reinterpret_cast<const Real *>(p->Aop64);
        with_tables<Real, GRIDS, RK4>(p, [&](const Real *fl, const Real *cs, const Real *sn, auto... o)
                                      { with_flags([&](auto FORCED, auto HOLD)
                                                   { hipLaunchKernelGGL((ddh_mfma_kernel<Real, FORCED.value, HOLD.value, decltype(o)...>), launch_grid(p, n_local),
                                                                        dim3(p->launch.block), 0, st, A, K, fl, cs, sn, o...); },
                                                   A.x != nullptr, A.prio != 0); });
    }

    // kernel 5's element-lane form (LAST_COPY: form 3; PAIRED: chain order 2) and kernel 13 at n_basis 4
    template <bool LAST_COPY, bool PAIRED, bool GRIDS>
    void run_element_lane(const cuddh_ddh_plan *p, const DdhArgs<float> &A, int n_local, hipStream_t st)
    {
        with_tables<float, GRIDS, false>(p, [&](const float *fl, const float *cs, const float *sn, auto... o)
                                         { with_flags([&](auto FORCED, auto HOLD)
                                                      { hipLaunchKernelGGL((ddh_element_lane_kernel<FORCED.value, HOLD.value, LAST_COPY, PAIRED, decltype(o)...>),
                                                                           launch_grid(p, n_local), dim3(p->launch.block), 0, st, A, p->Sep4, fl, cs, sn, o...); },
                                                      A.x != nullptr, A.prio != 0); });
    }

    template <bool LAST_COPY, bool GRIDS>
    void run_element_lane8(const cuddh_ddh_plan *p, const DdhArgs<float> &A, int n_local, hipStream_t st) // kernel 11
    {
        with_tables<float, GRIDS, false>(p, [&](const float *fl, const float *cs, const float *sn, auto... o)
                                         { with_flags([&](auto FORCED, auto HOLD)
                                                      { hipLaunchKernelGGL((ddh_element_lane8_kernel<FORCED.value, HOLD.value, LAST_COPY, decltype(o)...>),
                                                                           launch_grid(p, n_local), dim3(p->launch.block), 0, st, A, p->Sep4, fl, cs, sn, o...); },
                                                      A.x != nullptr, A.prio != 0); });
    }

    template <bool LAST_COPY, bool GRIDS>
    void run_element_lane5(const cuddh_ddh_plan *p, const DdhArgs<float> &A, int n_local, hipStream_t st) // kernel 12, and 13 at n_basis 5
    {
        with_tables<float, GRIDS, false>(p, [&](const float *fl, const float *cs, const float *sn, auto... o)
                                         { with_flags([&](auto FORCED, auto HOLD)
                                                      { hipLaunchKernelGGL((ddh_element_lane5_kernel<FORCED.value, HOLD.value, LAST_COPY, decltype(o)...>),
                                                                           launch_grid(p, n_local), dim3(p->launch.block), 0, st, A, p->Sep4, fl, cs, sn, o...); },
                                                      A.x != nullptr, A.prio != 0); });
    }

    // The launch of kernel r.kernel in the plan's state.  Only combinations that are launched are instantiated: kernels 3, 4,
    // 7 and the folded-DPP form of 9 in fp32 only (fp64 takes the plain form), 5 and the element-lane kernels in fp32 and 8 in
    // fp64 only, no RK4 form of 3, 4, 11 and 13, and 6, 7, 12 and the element-lane form of 5 on one time grid with RK2 alone.
    // ddh_resolve() never resolves to the others; if it did, L.run* would stay null and resolve() would refuse the plan.
    template <typename Real, bool GRIDS, bool RK4>
    void set_launch(const cuddh_ddh_plan *p, const DdhResolved &r, DdhLaunch &L)
    {
        constexpr bool f32 = sizeof(Real) == 4, plain = !GRIDS && !RK4;
        DdhRun<Real> run = nullptr;
        const bool last_copy = p->last_copy != 0;
        switch (r.kernel)
        {
        case 1:
        case 10: // one workgroup per subdomain, one thread per element node; 52 KB of LDS in fp64 at 1024 nodes: within the 64 KB
                 // a workgroup gets without asking
            L.per_group = 1;
            L.block = p->nodes;
            L.lds = (size_t)p->nodes * (4 * sizeof(Real) + 5 * sizeof(int));
            with_n_basis(p->d.nb, [&](auto NB)
                         {
                             if (p->nodes <= 256)
                                 run = r.kernel == 10 ? run_block<Real, NB.value, true, 256, GRIDS, RK4> : run_block<Real, NB.value, false, 256, GRIDS, RK4>;
                             else if (r.kernel == 1 && p->nodes <= 1024)
                                 run = run_block<Real, NB.value, false, 1024, GRIDS, RK4>;
                         });
            break;
        case 2: run = run_wave<Real, 0, GRIDS, RK4>; break;
        case 3:
            if constexpr (!RK4)
                run = run_wave<Real, f32 ? 1 : 0, GRIDS, RK4>;
            break;
        case 4:
            if constexpr (!RK4)
                run = run_wave<Real, f32 ? 2 : 0, GRIDS, RK4>;
            break;
        case 5:
            if constexpr (f32)
            {
                if (r.form < 2)
                    run = run_mfma<float, GRIDS, RK4>;
                else if constexpr (plain)
                {
                    L.per_group = 16; // four subdomains per wavefront
                    with_flags([&](auto LAST_COPY, auto PAIRED) { run = run_element_lane<LAST_COPY.value, PAIRED.value, false>; }, r.form == 3, r.order == 2);
                }
            }
            break;
        case 8:
            if constexpr (!f32)
                run = run_mfma<double, GRIDS, RK4>;
            break;
        case 6:
        case 7:
            if constexpr (plain)
            {
                L.per_group = 8; // two subdomains per wavefront
                if constexpr (f32)
                    run = r.kernel == 7 ? run_wave8<float, true, true> : run_wave8<float, true, false>;
                else if (r.kernel == 6)
                    run = run_wave8<double, false, false>;
            }
            break;
        case 9: run = run_general_wave<Real, f32 ? 1 : 0, GRIDS, RK4>; break;
        case 11:
            if constexpr (f32 && !RK4)
                with_flags([&](auto LAST_COPY) { run = run_element_lane8<LAST_COPY.value, GRIDS>; }, last_copy);
            break;
        case 12:
            if constexpr (f32 && plain)
            {
                L.per_group = 16;
                with_flags([&](auto LAST_COPY) { run = run_element_lane5<LAST_COPY.value, false>; }, last_copy);
            }
            break;
        case 13: // the element-lane kernels with four subdomains per wavefront, with or without time grids; RK2 only
            if constexpr (f32 && !RK4)
            {
                L.per_group = 16;
                with_flags(
                    [&](auto LAST_COPY)
                    {
                        if (p->d.nb == 4)
                            run = run_element_lane<LAST_COPY.value, false, GRIDS>;
                        else
                            run = run_element_lane5<LAST_COPY.value, GRIDS>;
                    },
                    last_copy);
            }
            break;
        }
        if constexpr (f32)
            L.run32 = run;
        else
            L.run64 = run;
    }

    // What the plan runs, from its facts and options as they stand (ddh_resolve) and the launch that goes with it.  `setting`:
    // the option the calling setter has just stored (DdhSetting).  On refusal the record is left as it was.
    int resolve(cuddh_ddh_plan *p, int setting = DDH_SET_NONE)
    {
        const DdhShape shape{p->d.nb, p->d.nel1d, p->d.n_domains, p->is_f64, p->mx_elems};
        DdhResolved r;
        if (ddh_resolve(shape, p->requested, p->facts, p->now.kernel, DdhOptions{p->n_grids > 0, p->rk4, p->sweep_form, p->chain_order}, setting, r))
            return static_cast<int>(hipErrorInvalidValue);
        DdhLaunch L;
        with_flags([&](auto F64, auto GRIDS, auto RK4) { set_launch<std::conditional_t<F64.value, double, float>, GRIDS.value, RK4.value>(p, r, L); },
                   p->is_f64 != 0, p->n_grids > 0, p->rk4 != 0);
        if (!L.run32 && !L.run64) // a missing kernel is an error
            return static_cast<int>(hipErrorInvalidValue);
        p->now = r;
        p->launch = L;
        return 0;
    }

    // A setter: stores its option (store(plan)), resolves, and on refusal puts the plan back as it was.
    template <class Store>
    int set_and_resolve(cuddh_ddh_plan *p, int setting, Store store)
    {
        const cuddh_ddh_plan before = *p;
        store(*p);
        const int err = resolve(p, setting);
        if (err)
            *p = before;
        return err;
    }

    template <typename Real>
    int apply(const cuddh_ddh_plan *plan, const int *dom_list, int dom_begin, int dom_end, const double *x, double *y, int zero_y, const Real *lambda,
              Real *update, void *stream)
    {
        if (!plan || plan->is_f64 != (sizeof(Real) == 8 ? 1 : 0))
            return static_cast<int>(hipErrorInvalidValue);
        const cuddh_ddh_desc &d = plan->d;
        if (dom_begin < 0 || (!dom_list && dom_end > d.n_domains) || dom_begin > dom_end)
            return static_cast<int>(hipErrorInvalidValue);
        hipStream_t st = as_stream(stream);
        const int g_ndof = plan->gI_override ? plan->g_ndof_override : d.g_ndof;
        if (y && zero_y)
        {
            hipError_t e = hipMemsetAsync(y, 0, (size_t)2 * g_ndof * sizeof(double), st);
            if (e != hipSuccess)
                return static_cast<int>(e);
        }
        const int n_local = dom_end - dom_begin;
        if (n_local == 0)
            return 0;
        // all subdomains of a plan with time grids: the long ones first, so that the short ones fill the device behind them
        // instead of a few long ones running on alone at the end.  Caller lists run in the caller's order, and so do ranges,
        // through the plan's identity list (domain_at: a launch of such a plan always has a list).
        if (plan->n_grids > 0 && !dom_list)
        {
            dom_list = dom_begin == 0 && dom_end == d.n_domains ? plan->by_steps : plan->by_index + dom_begin;
            dom_begin = 0;
            dom_end = n_local;
        }

        DdhArgs<Real> A;
        A.g_ndof = g_ndof;
        A.n_lambda = d.n_lambda;
        A.nt = d.nt;
        A.wh_iters = plan->wh_iters;
        A.prio = plan->wave_priority;
        A.mx_dof = d.mx_dof;
        A.mx_fdof = d.mx_fdof;
        A.nodes = plan->nodes;
        A.dom_begin = dom_begin;
        A.dom_end = dom_end;
        A.dom_list = dom_list;
        A.omega = static_cast<Real>(d.omega);
        A.dt = static_cast<Real>(d.dt);
        A.s_dof = d.s_dof;
        A.s_fdof = d.s_fdof;
        A.B = d.B;
        A.gI = plan->gI_override ? plan->gI_override : d.gI;
        A.sI = d.sI;
        A.G = static_cast<const Real *>(d.G);
        A.m = static_cast<const Real *>(d.m);
        A.gmi = static_cast<const Real *>(d.gmi);
        A.a = static_cast<const Real *>(d.a);
        A.H = static_cast<const Real *>(d.H);
        A.x = x;
        A.y = y;
        A.lambda = lambda;
        A.update = update;
        A.csr_off = plan->csr_off;
        A.csr_src = plan->csr_src;
        A.unique_y = plan->gI_override ? 1 : 0;

        if constexpr (sizeof(Real) == 4)
            plan->launch.run32(plan, A, n_local, st);
        else
            plan->launch.run64(plan, A, n_local, st);
        return launch_status();
    }
} // namespace

extern "C"
{
    int cuddh_hip_ddh_geom_setup_f32(int n_domains, int mx_elems, int g_elem, int nb, const int *n_elems, const int *elems,
                                     const double *w, const double *J, float *G, void *stream)
    {
        (void)g_elem;
        return geom_setup<float>(n_domains, mx_elems, nb, n_elems, elems, w, J, nullptr, nullptr, G, stream);
    }

    int cuddh_hip_ddh_geom_setup_f64(int n_domains, int mx_elems, int g_elem, int nb, const int *n_elems, const int *elems,
                                     const double *w, const double *J, double *G, void *stream)
    {
        (void)g_elem;
        return geom_setup<double>(n_domains, mx_elems, nb, n_elems, elems, w, J, nullptr, nullptr, G, stream);
    }

    int cuddh_hip_ddh_geom_from_corners_f32(int n_domains, int mx_elems, int nb, const int *n_elems, const int *elems, const double *w,
                                            const double *points, const double *corners, float *G, void *stream)
    {
        if (!corners || !points)
            return static_cast<int>(hipErrorInvalidValue);
        return geom_setup<float>(n_domains, mx_elems, nb, n_elems, elems, w, nullptr, corners, points, G, stream);
    }

    int cuddh_hip_ddh_geom_from_corners_f64(int n_domains, int mx_elems, int nb, const int *n_elems, const int *elems, const double *w,
                                            const double *points, const double *corners, double *G, void *stream)
    {
        if (!corners || !points)
            return static_cast<int>(hipErrorInvalidValue);
        return geom_setup<double>(n_domains, mx_elems, nb, n_elems, elems, w, nullptr, corners, points, G, stream);
    }

    int cuddh_hip_ddh_plan_create(cuddh_ddh_plan **out, const cuddh_ddh_desc *desc, int is_f64, int kernel)
    {
        *out = nullptr;
        if (!desc)
            return static_cast<int>(hipErrorInvalidValue);
        // the checks this shape and request call for; < 0: a shape no kernel takes, or a kernel requested on a shape not its own
        const int checks = ddh_checks(DdhShape{desc->nb, desc->nel1d, desc->n_domains, is_f64 ? 1 : 0, 0}, kernel);
        if (checks < 0)
            return static_cast<int>(hipErrorInvalidValue);

        cuddh_ddh_plan *p = new cuddh_ddh_plan;
        p->d = *desc;
        p->is_f64 = is_f64 ? 1 : 0;
        p->nodes = desc->nb * desc->nb * desc->nel1d * desc->nel1d;
        p->requested = kernel;
        int err = is_f64 ? establish_facts<double>(p, checks) : establish_facts<float>(p, checks);
        if (!err)
            err = resolve(p); // refused: a requested kernel one of whose checks did not hold
        if (err)
        {
            cuddh_hip_ddh_plan_destroy(p);
            return err;
        }
        *out = p;
        return 0;
    }

    int cuddh_hip_ddh_plan_create_general(cuddh_ddh_plan **out, const cuddh_ddh_desc *desc, int mx_elems, int is_f64, int kernel)
    {
        if (!out)
            return static_cast<int>(hipErrorInvalidValue);
        *out = nullptr;
        static_assert(GW_NODES == DDH_GENERAL_MAX_NODES, "ddh_resolve.hpp holds the node count kernel 9 is built for");
        if (!desc || desc->n_domains < 1 || mx_elems < 1 || ddh_checks(DdhShape{desc->nb, 0, desc->n_domains, is_f64 ? 1 : 0, mx_elems}, kernel) < 0)
            return static_cast<int>(hipErrorInvalidValue);
        const int nb = desc->nb, nodes = nb * nb * mx_elems;
        if (desc->mx_dof > nodes || desc->mx_fdof > desc->mx_dof)
            return static_cast<int>(hipErrorInvalidValue);

        // assembly lists from sI, checked entry by entry on the host: nothing the kernels index with is left unchecked
        const int nd = desc->n_domains;
        std::vector<int> sI((size_t)nodes * nd), s_dof(nd), s_fdof(nd);
        hipError_t e = hipMemcpy(sI.data(), desc->sI, sizeof(int) * sI.size(), hipMemcpyDeviceToHost);
        if (e == hipSuccess)
            e = hipMemcpy(s_dof.data(), desc->s_dof, sizeof(int) * nd, hipMemcpyDeviceToHost);
        if (e == hipSuccess)
            e = hipMemcpy(s_fdof.data(), desc->s_fdof, sizeof(int) * nd, hipMemcpyDeviceToHost);
        if (e != hipSuccess)
            return static_cast<int>(e);
        std::vector<int> off((size_t)(nodes + 1) * nd, 0), src((size_t)nodes * nd, 0);
        for (int s = 0; s < nd; ++s)
        {
            const int ndof = s_dof[s];
            if (ndof < 1 || ndof > desc->mx_dof || s_fdof[s] < 0 || s_fdof[s] > ndof || s_fdof[s] > desc->mx_fdof)
                return static_cast<int>(hipErrorInvalidValue);
            const int *I = sI.data() + (size_t)nodes * s;
            int *o = off.data() + (size_t)(nodes + 1) * s, *c = src.data() + (size_t)nodes * s;
            for (int n = 0; n < nodes; ++n)
            {
                if (I[n] < -1 || I[n] >= ndof)
                    return static_cast<int>(hipErrorInvalidValue);
                if (I[n] >= 0)
                    ++o[I[n] + 1];
            }
            for (int dd = 0; dd < nodes; ++dd)
            {
                if (dd < ndof && o[dd + 1] == 0)
                    return static_cast<int>(hipErrorInvalidValue); // a dof no element node maps to
                o[dd + 1] += o[dd];
            }
            std::vector<int> fill(o, o + nodes);
            for (int n = 0; n < nodes; ++n) // ascending element node: the summation order of kernel 1
                if (I[n] >= 0)
                    c[fill[I[n]]++] = n;
        }

        cuddh_ddh_plan *p = new cuddh_ddh_plan;
        p->d = *desc;
        p->is_f64 = is_f64 ? 1 : 0;
        p->nodes = nodes;
        p->mx_elems = mx_elems;
        p->requested = kernel;
        e = hipMalloc(reinterpret_cast<void **>(&p->csr_off), sizeof(int) * off.size());
        if (e == hipSuccess)
            e = hipMalloc(reinterpret_cast<void **>(&p->csr_src), sizeof(int) * src.size());
        if (e == hipSuccess)
            e = hipMemcpy(p->csr_off, off.data(), sizeof(int) * off.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMemcpy(p->csr_src, src.data(), sizeof(int) * src.size(), hipMemcpyHostToDevice);
        const int err = e != hipSuccess ? static_cast<int>(e) : resolve(p);
        if (err)
        {
            cuddh_hip_ddh_plan_destroy(p);
            return err;
        }
        *out = p;
        return 0;
    }

    int cuddh_hip_ddh_plan_destroy(cuddh_ddh_plan *plan)
    {
        if (plan && plan->csr_off)
            (void)hipFree(plan->csr_off);
        if (plan && plan->csr_src)
            (void)hipFree(plan->csr_src);
        if (plan && plan->Aop)
            (void)hipFree(plan->Aop);
        if (plan && plan->Aop64)
            (void)hipFree(plan->Aop64);
        if (plan && plan->Sep)
            (void)hipFree(plan->Sep);
        if (plan && plan->Sep4)
            (void)hipFree(plan->Sep4);
        if (plan && plan->grids)
            (void)hipFree(plan->grids);
        if (plan && plan->by_steps)
            (void)hipFree(plan->by_steps);
        if (plan && plan->by_index)
            (void)hipFree(plan->by_index);
        delete plan;
        return 0;
    }

    int cuddh_hip_ddh_plan_kernel(const cuddh_ddh_plan *plan) { return plan ? plan->now.kernel : 0; }

    int cuddh_hip_ddh_plan_set_vector_layout(cuddh_ddh_plan *plan, const int *d_gI, int g_ndof)
    {
        if (!plan || (d_gI && g_ndof <= 0))
            return static_cast<int>(hipErrorInvalidValue);
        plan->gI_override = d_gI;
        plan->g_ndof_override = d_gI ? g_ndof : 0;
        return 0;
    }

    int cuddh_hip_ddh_plan_set_wave_priority(cuddh_ddh_plan *plan, int high)
    {
        if (!plan)
            return static_cast<int>(hipErrorInvalidValue);
        plan->wave_priority = high ? 1 : 0;
        return 0;
    }

    int cuddh_hip_ddh_plan_set_wh_iters(cuddh_ddh_plan *plan, int wh_iters)
    {
        if (!plan || wh_iters < 0)
            return static_cast<int>(hipErrorInvalidValue);
        plan->wh_iters = wh_iters == 0 ? WH_ITERS_REFERENCE : wh_iters;
        return 0;
    }

    // The setters below store their argument, resolve, and on refusal leave the plan as it was (set_and_resolve); which values
    // a plan takes is ddh_resolve's to say.
    int cuddh_hip_ddh_plan_set_sweep_form(cuddh_ddh_plan *plan, int form)
    {
        if (!plan)
            return static_cast<int>(hipErrorInvalidValue);
        return set_and_resolve(plan, DDH_SET_SWEEP_FORM, [&](cuddh_ddh_plan &p) { p.sweep_form = form; });
    }

    int cuddh_hip_ddh_plan_sweep_form(const cuddh_ddh_plan *plan) { return plan ? plan->now.form : 0; }

    int cuddh_hip_ddh_plan_set_chain_order(cuddh_ddh_plan *plan, int order)
    {
        if (!plan)
            return static_cast<int>(hipErrorInvalidValue);
        return set_and_resolve(plan, DDH_SET_CHAIN_ORDER, [&](cuddh_ddh_plan &p) { p.chain_order = order; });
    }

    int cuddh_hip_ddh_plan_chain_order(const cuddh_ddh_plan *plan) { return plan ? plan->now.order : 0; }

    int cuddh_hip_ddh_plan_set_time_grids(cuddh_ddh_plan *plan, int n_grids, const int *h_nt, const double *h_dt, const void *filter,
                                          const void *cs, const void *sn, const int *d_grid_of)
    {
        if (!plan || n_grids < 1 || !h_nt || !h_dt || !filter || !cs || !sn || !d_grid_of)
            return static_cast<int>(hipErrorInvalidValue);
        const int nd = plan->d.n_domains;
        // every offset a kernel adds to a table base is formed and checked here
        std::vector<int> filt_off(n_grids), cs_off(n_grids);
        long long fo = 0, co = 0;
        for (int g = 0; g < n_grids; ++g)
        {
            if (h_nt[g] < 1 || !(h_dt[g] > 0.0) || !std::isfinite(h_dt[g]))
                return static_cast<int>(hipErrorInvalidValue);
            filt_off[g] = static_cast<int>(fo);
            cs_off[g] = static_cast<int>(co);
            fo += (long long)h_nt[g] + 1;
            co += 2LL * h_nt[g] + 1;
            if (co > 2147483647LL)
                return static_cast<int>(hipErrorInvalidValue);
        }
        std::vector<int> grid_of(nd);
        hipError_t e = hipMemcpy(grid_of.data(), d_grid_of, sizeof(int) * nd, hipMemcpyDeviceToHost);
        if (e != hipSuccess)
            return static_cast<int>(e);
        for (int s = 0; s < nd; ++s)
            if (grid_of[s] < 0 || grid_of[s] >= n_grids)
                return static_cast<int>(hipErrorInvalidValue);
        std::vector<int> order(nd);
        for (int s = 0; s < nd; ++s)
            order[s] = s;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return h_nt[grid_of[a]] > h_nt[grid_of[b]]; });

        std::vector<int> index(nd);
        for (int s = 0; s < nd; ++s)
            index[s] = s;
        void *d_grids = nullptr;
        int *d_order = nullptr, *d_index = nullptr;
        auto upload_grids = [&](auto real)
        {
            using Real = decltype(real);
            std::vector<DdhTimeGrid<Real>> h(n_grids);
            for (int g = 0; g < n_grids; ++g)
                h[g] = {h_nt[g], filt_off[g], cs_off[g], static_cast<Real>(h_dt[g])};
            hipError_t err = hipMalloc(&d_grids, sizeof(DdhTimeGrid<Real>) * n_grids);
            if (err == hipSuccess)
                err = hipMemcpy(d_grids, h.data(), sizeof(DdhTimeGrid<Real>) * n_grids, hipMemcpyHostToDevice);
            return err;
        };
        e = plan->is_f64 ? upload_grids(double()) : upload_grids(float());
        if (e == hipSuccess)
            e = hipMalloc(reinterpret_cast<void **>(&d_order), sizeof(int) * nd);
        if (e == hipSuccess)
            e = hipMemcpy(d_order, order.data(), sizeof(int) * nd, hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMalloc(reinterpret_cast<void **>(&d_index), sizeof(int) * nd);
        if (e == hipSuccess)
            e = hipMemcpy(d_index, index.data(), sizeof(int) * nd, hipMemcpyHostToDevice);
        if (e != hipSuccess)
        {
            if (d_grids)
                (void)hipFree(d_grids);
            if (d_order)
                (void)hipFree(d_order);
            if (d_index)
                (void)hipFree(d_index);
            return static_cast<int>(e);
        }
        // The kernels that hold one subdomain per wavefront or workgroup take the grids as they are, and so does kernel 13, which
        // marches once per grid among its four (GroupedRows); 6, 7 and 12 chosen by auto give way to kernel 1, requested they
        // are refused, as is a plan with sweep form 2 or 3 set (ddh_resolve).
        void *const old_grids = plan->grids, *const old_steps = plan->by_steps, *const old_index = plan->by_index;
        const int err = set_and_resolve(plan, DDH_SET_NONE,
                                        [&](cuddh_ddh_plan &p)
                                        {
                                            p.grids = d_grids;
                                            p.by_steps = d_order;
                                            p.by_index = d_index;
                                            p.n_grids = n_grids;
                                            p.grid_of = d_grid_of;
                                            p.grid_filter = filter;
                                            p.grid_cs = cs;
                                            p.grid_sn = sn;
                                        });
        for (void *gone : {err ? d_grids : old_grids, err ? static_cast<void *>(d_order) : old_steps, err ? static_cast<void *>(d_index) : old_index})
            if (gone)
                (void)hipFree(gone);
        return err;
    }

    int cuddh_hip_ddh_plan_time_grids(const cuddh_ddh_plan *plan) { return plan ? plan->n_grids : 0; }

    // RK4 on a kernel without the form: a request is refused; an auto choice moves to the kernel of its block size that has
    // one, and scheme 0 afterwards leaves it there: results depend on the scheme, not on the kernel (ddh_resolve)
    int cuddh_hip_ddh_plan_set_integrator(cuddh_ddh_plan *plan, int scheme)
    {
        if (!plan || scheme < 0 || scheme > 1)
            return static_cast<int>(hipErrorInvalidValue);
        return set_and_resolve(plan, DDH_SET_NONE, [&](cuddh_ddh_plan &p) { p.rk4 = scheme; });
    }

    int cuddh_hip_ddh_plan_integrator(const cuddh_ddh_plan *plan) { return plan ? plan->rk4 : 0; }

    int cuddh_hip_ddh_plan_set_owner_rule(cuddh_ddh_plan *plan, int last)
    {
        if (!plan)
            return static_cast<int>(hipErrorInvalidValue);
        return set_and_resolve(plan, DDH_SET_OWNER_RULE, [&](cuddh_ddh_plan &p) { p.last_copy = last ? 1 : 0; });
    }

    int cuddh_hip_ddh_apply_f32(const cuddh_ddh_plan *plan, int dom_begin, int dom_end, const double *x, double *y, int zero_y,
                                const float *lambda, float *update, void *stream)
    {
        return apply<float>(plan, nullptr, dom_begin, dom_end, x, y, zero_y, lambda, update, stream);
    }

    int cuddh_hip_ddh_apply_list_f32(const cuddh_ddh_plan *plan, const int *d_domains, int n, const double *x, double *y, int zero_y,
                                     const float *lambda, float *update, void *stream)
    {
        if (!d_domains && n > 0)
            return static_cast<int>(hipErrorInvalidValue);
        return apply<float>(plan, d_domains, 0, n, x, y, zero_y, lambda, update, stream);
    }

    int cuddh_hip_ddh_apply_list_f64(const cuddh_ddh_plan *plan, const int *d_domains, int n, const double *x, double *y, int zero_y,
                                     const double *lambda, double *update, void *stream)
    {
        if (!d_domains && n > 0)
            return static_cast<int>(hipErrorInvalidValue);
        return apply<double>(plan, d_domains, 0, n, x, y, zero_y, lambda, update, stream);
    }

    int cuddh_hip_ddh_apply_f64(const cuddh_ddh_plan *plan, int dom_begin, int dom_end, const double *x, double *y, int zero_y,
                                const double *lambda, double *update, void *stream)
    {
        return apply<double>(plan, nullptr, dom_begin, dom_end, x, y, zero_y, lambda, update, stream);
    }
}
