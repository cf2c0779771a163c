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
//   * `ddh_element_lane_kernel<5, ..>` (n_basis == 5, 4x4 elements, rectangles) runs four
//     subdomains per wavefront, lane = element with its 25 nodes in registers:
//     both contractions in-lane, assembly by DPP row shifts inside a 16-lane row;
//   * `ddh_block_kernel` (any n_basis <= 10) runs one subdomain per workgroup
//     with the field staged in LDS, 3 barriers per stiffness sweep.
//
// Shape of the file: one translation unit in three files.  ddh_device.hpp, included first, holds what every kernel is
// built from: DdhArgs, the time grids, the scheme tags and the local solve around a sweep; ddh_element_lane.hpp the
// element-lane family (kernels 5 in its element-lane form, 11, 12 and 13); this file the other kernels, the plan and
// the launches.  The build's per-file flags for ddh.hip therefore hold for all three.
// Every local solve is  load_dof (per-dof coefficients)  ->
// wh_march (the WaveHoltz time stepping, RK2 or for an RK4 plan RK4, around a callable `sweep(w, z)`,
// z = S w)  ->  publish_dof (y and the trace update).  All six wavefront kernels
// use load_dof.  ddh_wave8_kernel, ddh_mfma_kernel<Real, ..> and
// ddh_element_lane_kernel<NB, ..> (one element per lane, four subdomains per wavefront: kernel 5's second sweep form
// at NB = 4, kernel 12 at NB = 5 with 25 nodes per lane, one frame for both) and ddh_element_lane8_kernel (kernel 11:
// the same with one 8x8-element subdomain per wavefront) use wh_march and publish_dof too and are a lane
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

#include "ddh_device.hpp"
#include "ddh_element_lane.hpp"
#include "ddh_resolve.hpp"
#include "element_lane_tables.hpp"

using namespace cuddh_k;

struct cuddh_ddh_plan;

namespace
{
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
    //  8x8 elements, fp32: one element per lane, one subdomain per wavefront);  12 ddh_element_lane_kernel<5, ..> (nb == 5, 4x4
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
    int forcing = 0; // the same form's march: 0 auto, 1 the trace sources in every WaveHoltz pass, 2 in the first only (cuddh_hip_ddh_plan_set_forcing)
    int forcing_now = 0; // the forcing in effect (ddh_forcing), filled by resolve() beside `now`
    int march = 0; // how that march carries the velocity: 0 auto, 1 as it is, 2 scaled, its midpoint update in the sweep (cuddh_hip_ddh_plan_set_march)
    int march_now = 0; // the march in effect (ddh_march), filled by resolve() beside `now`
    int head = 0; // what march 2 carries as the velocity: 0 auto, 1 q / (2 hm), 2 that times the first chain's head coefficient (cuddh_hip_ddh_plan_set_head)
    int head_now = 0; // the head in effect (ddh_head), filled by resolve() beside `now`
    int assembly = 0; // how head 2 forms the sweep's neighbour sums: 0 auto, 1 DPP, 2 fetched both ways over the LDS pipe (cuddh_hip_ddh_plan_set_assembly)
    int assembly_now = 0; // the assembly in effect (ddh_assembly), filled by resolve() beside `now`
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

    // Issue priority of the calling wavefront (s_setprio).  All wavefronts of one rank's local solves are resident at once and
    // advance at the same rate, so a launch of the few subdomains whose traces other ranks wait for finishes no earlier than
    // the launch of all the others it shares the SIMDs with (profiles/r02/overlap_timeline.txt) -- unless its wavefronts are
    // issued first whenever they are ready.
    __device__ inline void raise_priority(int prio)
    {
        if (prio)
            __builtin_amdgcn_s_setprio(3);
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

    // the row-per-subdomain element-lane kernel.  NB 4: kernel 5's element-lane form (LAST_COPY: form 3; PAIRED: chain order 2)
    // and kernel 13 at n_basis 4;  NB 5: kernel 12, and 13 at n_basis 5.  Sep4 holds the plan's table at either order
    template <int NB, bool LAST_COPY, bool PAIRED, bool ONCE, bool SCALED, bool CARRIED, bool FETCHED, bool GRIDS>
    void run_element_lane(const cuddh_ddh_plan *p, const DdhArgs<float> &A, int n_local, hipStream_t st)
    {
        with_tables<float, GRIDS, false>(p, [&](const float *fl, const float *cs, const float *sn, auto... o)
                                         { with_flags([&](auto FORCED, auto HOLD)
                                                      { hipLaunchKernelGGL((ddh_element_lane_kernel<NB, FORCED.value, HOLD.value, LAST_COPY, PAIRED, ONCE, SCALED, CARRIED, FETCHED, decltype(o)...>),
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

    // The launch of kernel r.kernel in the plan's state.  Only combinations that are launched are instantiated: kernels 3, 4,
    // 7 and the folded-DPP form of 9 in fp32 only (fp64 takes the plain form), 5 and the element-lane kernels in fp32 and 8 in
    // fp64 only, no RK4 form of 3, 4, 11 and 13, and 6, 7, 12 and the element-lane form of 5 on one time grid with RK2 alone.
    // ddh_resolve() never resolves to the others; if it did, L.run* would stay null and resolve() would refuse the plan.
    template <typename Real, bool GRIDS, bool RK4>
    void set_launch(const cuddh_ddh_plan *p, const DdhResolved &r, int forcing, int march, int head, int assembly, DdhLaunch &L)
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
                    // the sources in the first pass only (forcing 2) exist beside the paired chains alone, and ddh_forcing gives 2 there alone;
                    // the scaled march (march 2) beside forcing 2 alone, and ddh_march gives 2 there alone; the carried head (head 2)
                    // beside march 2 alone, and ddh_head gives 2 there alone
                    // the assembly over the LDS pipe (assembly 2) beside head 2 alone, and ddh_assembly gives 2 there alone
                    with_flags([&](auto LAST_COPY, auto PAIRED, auto ONCE, auto SCALED, auto CARRIED, auto FETCHED)
                               {
                                   constexpr bool once = PAIRED.value && ONCE.value, scaled = once && SCALED.value, carried = scaled && CARRIED.value;
                                   run = run_element_lane<4, LAST_COPY.value, PAIRED.value, once, scaled, carried, carried && FETCHED.value, false>;
                               },
                               r.form == 3, r.order == 2, forcing == 2, march == 2, head == 2, assembly == 2);
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
                with_flags([&](auto LAST_COPY) { run = run_element_lane<5, LAST_COPY.value, false, false, false, false, false, false>; }, last_copy);
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
                            run = run_element_lane<4, LAST_COPY.value, false, false, false, false, false, GRIDS>;
                        else
                            run = run_element_lane<5, LAST_COPY.value, false, false, false, false, false, GRIDS>;
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
        if (setting == DDH_SET_FORCING && ddh_forcing_accepted(shape, p->requested, p->facts, p->now.kernel,
                                                               DdhOptions{p->n_grids > 0, p->rk4, p->sweep_form, p->chain_order}, p->forcing))
            return static_cast<int>(hipErrorInvalidValue);
        if (setting == DDH_SET_MARCH && ddh_march_accepted(shape, p->requested, p->facts, p->now.kernel,
                                                           DdhOptions{p->n_grids > 0, p->rk4, p->sweep_form, p->chain_order}, p->march))
            return static_cast<int>(hipErrorInvalidValue);
        if (setting == DDH_SET_HEAD && ddh_head_accepted(shape, p->requested, p->facts, p->now.kernel,
                                                         DdhOptions{p->n_grids > 0, p->rk4, p->sweep_form, p->chain_order}, p->head))
            return static_cast<int>(hipErrorInvalidValue);
        const int forcing = ddh_forcing(r, p->sweep_form, p->chain_order, p->forcing);
        const int march = ddh_march(forcing, p->sweep_form, p->chain_order, p->forcing, p->march);
        const int head = ddh_head(march, p->head);
        if (setting == DDH_SET_ASSEMBLY && ddh_assembly_accepted(head, p->assembly))
            return static_cast<int>(hipErrorInvalidValue);
        const int assembly = ddh_assembly(head, p->d.n_domains, p->assembly);
        DdhLaunch L;
        with_flags([&](auto F64, auto GRIDS, auto RK4) { set_launch<std::conditional_t<F64.value, double, float>, GRIDS.value, RK4.value>(p, r, forcing, march, head, assembly, L); },
                   p->is_f64 != 0, p->n_grids > 0, p->rk4 != 0);
        if (!L.run32 && !L.run64) // a missing kernel is an error
            return static_cast<int>(hipErrorInvalidValue);
        p->now = r;
        p->forcing_now = forcing;
        p->march_now = march;
        p->head_now = head;
        p->assembly_now = assembly;
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

    int cuddh_hip_ddh_plan_set_forcing(cuddh_ddh_plan *plan, int forcing)
    {
        if (!plan)
            return static_cast<int>(hipErrorInvalidValue);
        return set_and_resolve(plan, DDH_SET_FORCING, [&](cuddh_ddh_plan &p) { p.forcing = forcing; });
    }

    int cuddh_hip_ddh_plan_forcing(const cuddh_ddh_plan *plan) { return plan ? plan->forcing_now : 0; }

    int cuddh_hip_ddh_plan_set_march(cuddh_ddh_plan *plan, int march)
    {
        if (!plan)
            return static_cast<int>(hipErrorInvalidValue);
        return set_and_resolve(plan, DDH_SET_MARCH, [&](cuddh_ddh_plan &p) { p.march = march; });
    }

    int cuddh_hip_ddh_plan_march(const cuddh_ddh_plan *plan) { return plan ? plan->march_now : 0; }

    int cuddh_hip_ddh_plan_set_head(cuddh_ddh_plan *plan, int head)
    {
        if (!plan)
            return static_cast<int>(hipErrorInvalidValue);
        return set_and_resolve(plan, DDH_SET_HEAD, [&](cuddh_ddh_plan &p) { p.head = head; });
    }

    int cuddh_hip_ddh_plan_head(const cuddh_ddh_plan *plan) { return plan ? plan->head_now : 0; }

    int cuddh_hip_ddh_plan_set_assembly(cuddh_ddh_plan *plan, int assembly)
    {
        if (!plan)
            return static_cast<int>(hipErrorInvalidValue);
        return set_and_resolve(plan, DDH_SET_ASSEMBLY, [&](cuddh_ddh_plan &p) { p.assembly = assembly; });
    }

    int cuddh_hip_ddh_plan_assembly(const cuddh_ddh_plan *plan) { return plan ? plan->assembly_now : 0; }

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
