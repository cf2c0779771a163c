// The element-lane family of DDH local-solve kernels (one element per lane, its nodes in registers; fp32, rectangles), part
// of the one translation unit ddh.hip:
//   ddh_element_lane_kernel<NB, ..>  a subdomain of 4x4 elements per 16-lane DPP row, four per wavefront: kernel 5's
//                                    element-lane form (NB = 4, the packed time loop), kernel 12 (NB = 5, node by node) and,
//                                    with TimeGrids, kernel 13 for both.  ONE frame (early exit, pass loop, the two locates,
//                                    owner rule); what the two orders do differently stands under `if constexpr (NB == 4)`;
//   ddh_element_lane8_kernel         kernel 11: a subdomain of 8x8 elements per wavefront (NB = 4).
// Shared by all of them: the in-lane products, the interior masks, the folded weight W and the owner rule.  The DPP assembly
// statements exist per value count (4 and 5): their operand numbering and wait-state spacing are their content.
#ifndef CUDDH_AMD_DDH_ELEMENT_LANE_HPP
#define CUDDH_AMD_DDH_ELEMENT_LANE_HPP

#include <type_traits>

#include "ddh_device.hpp"

namespace
{
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
    // TimeGrids instantiations (kernel 13) and a form forced with set_sweep_form keep the pinned chains.  ONCE (forcing 2,
    // cuddh_hip_ddh_plan_set_forcing; what auto runs where it chose the form and the order) applies the trace sources in the
    // first WaveHoltz pass only (wh_march_pairs_once): 206 per wavefront-step in the later passes, both forms, 166 VGPRs, no
    // scratch, 32 KB of LDS per workgroup between the time loops; another new rounding (profiles/r28).  SCALED (march 2,
    // cuddh_hip_ddh_plan_set_march; what auto runs where it chose form, order and forcing) carries the velocity as q / (2 hm)
    // and folds its midpoint update into the head of the first sweep's chains, 1 / m of it in each of the m copies of a shared
    // node (wh_march_pairs_scaled): 226 per wavefront-step in the first pass and 198 in the later ones in the action form (230 to
    // 234 and 204 with x), 164 to 168 VGPRs, no scratch; one more new rounding (profiles/r31).
    // CARRIED (head 2, cuddh_hip_ddh_plan_set_head; what auto runs wherever march 2 is in effect) carries that velocity already
    // multiplied by the head coefficient of the first sweep's chain, so the chain opens on the state (wh_march_pairs_carried):
    // 214 and 190 in the action form (230 and 194 to 198 with x), 167 VGPRs, no scratch, 44 KB of LDS per workgroup, of which
    // 12 KB hold a per-dof coefficient that is read once per step, the only LDS access in a time loop of the family; one more
    // new rounding (profiles/r32).
    // FETCHED (assembly 2, cuddh_hip_ddh_plan_set_assembly; what auto runs where it chose all of the above) forms the neighbour
    // sums of head 2's sweeps over the LDS pipe: every copy of a shared node fetches the other copy's partial sum (ds_swizzle_b32,
    // no LDS storage) and adds it itself, a + b in one lane and b + a in the other, so the bits are those of the DPP assembly:
    // 16 fetches and 8 packed additions per sweep where there are 16 DPP instructions, 198 and 174 per wavefront-step in the
    // action form (208 and 176 with x), 167 VGPRs, no scratch (profiles/r33).
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
    // The same two for the five values a side of an n_basis-5 element holds (ddh_element_lane_kernel<5, ..>): the same instructions,
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

    // ---- what the kernels of the family share, for NB nodes per element side (4 or 5) and register n = k + NB l = node (k, l)
    // wh_march's INTERIOR for a lane that holds one node per register: the registers with 0 < k, l < NB - 1
    // (NB = 4: 5, 6, 9, 10; NB = 5: 6-8, 11-13, 16-18)
    constexpr unsigned element_interior_registers(int nb)
    {
        unsigned mask = 0;
        for (int l = 1; l < nb - 1; ++l)
            for (int k = 1; k < nb - 1; ++k)
                mask |= 1u << (k + nb * l);
        return mask;
    }

    // the in-lane part of the element-lane sweep: z' = Dg w + Bx-terms + By-terms of the lane's own element, before assembly
    template <int NB>
    __device__ inline void element_lane_products(const float (&w)[NB * NB], float (&z)[NB * NB], const float (&Bx)[NB * NB],
                                                 const float (&By)[NB * NB], const float (&Dg)[NB * NB])
    {
#pragma unroll
        for (int l = 0; l < NB; ++l)
#pragma unroll
            for (int k = 0; k < NB; ++k)
            {
                float t = Dg[k + NB * l] * w[k + NB * l];
#pragma unroll
                for (int j = 0; j < NB; ++j)
                {
                    if (j != k)
                        t += Bx[k + NB * j] * w[j + NB * l];
                    if (j != l)
                        t += By[l + NB * j] * w[k + NB * j];
                }
                z[k + NB * l] = t;
            }
    }

    // The node weight W folded into a dof's constants (z = W z': invm takes W, what stands beside z' is divided by it)
    __device__ inline void fold_weight(float W, float rW, float &invm, float &Hi, float &F, float &Gf)
    {
        invm *= W;
        Hi *= rW;
        F *= rW;
        Gf *= rW;
    }

    // The owner rule.  Every shared node is held by 2 or 4 (lane, register) pairs with identical values: the copy with the
    // smallest element-node index writes, with LAST_COPY the one with the largest.  Lane = ex + NEL ey in a subdomain of
    // NEL x NEL elements (4 or 8), whatever `tid` holds above those bits.
    template <int NB, int NEL, bool LAST_COPY>
    __device__ inline bool element_lane_owner(int n, int tid)
    {
        constexpr int EX = NEL - 1, EY = NEL * (NEL - 1); // the bits of ex and of NEL ey
        const int k = n % NB, l = n / NB;
        const bool first = !(k == 0 && (tid & EX) > 0) && !(l == 0 && (tid & EY) > 0);
        const bool last = !(k == NB - 1 && (tid & EX) < EX) && !(l == NB - 1 && (tid & EY) < EY);
        return LAST_COPY ? last : first;
    }
    // 1 / m, m the number of (lane, register) pairs that hold node n of this lane's element inside the subdomain (1, 2 or 4):
    // from the same (ex, ey, k, l) as the owner rule, so a node has more than one copy exactly where one of them does not own it
    template <int NB, int NEL>
    __device__ inline float element_lane_inverse_multiplicity(int n, int tid)
    {
        constexpr int EX = NEL - 1, EY = NEL * (NEL - 1);
        const int k = n % NB, l = n / NB;
        const bool two_x = (k == 0 && (tid & EX) > 0) || (k == NB - 1 && (tid & EX) < EX);
        const bool two_y = (l == 0 && (tid & EY) > 0) || (l == NB - 1 && (tid & EY) < EY);
        return (two_x ? 0.5f : 1.0f) * (two_y ? 0.5f : 1.0f);
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
    typedef __attribute__((address_space(3))) pair_t lds_pair_t; // a pair in LDS, named as such: ds_* with a 32-bit address
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

    // and for wh_march_pairs_once: its first pass as above in the action form and with no pair in the form with x (with the two
    // interior ones the instantiation with LAST_COPY spills 20 bytes); its time loop without sources, the same in both forms,
    // has the registers of F and Gf to spare and keeps dm in all eight
    constexpr unsigned ELEMENT_LANE_ONCE_FIRST_DM_PAIRS(bool forced) { return forced ? 0x00u : 0xffu; }
    constexpr unsigned ELEMENT_LANE_ONCE_DM_PAIRS = 0xffu;

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

    // The xi additions of the assembly over the LDS pipe, packed, two pairs a side: lo += what came from lane - 1 in the lanes with
    // ex > 0 (LANES 0xeeeeeeee), hi += what came from lane + 1 in the lanes with ex < 3 (0x77777777).  Which lanes add is the same in
    // every wavefront, so it is EXEC for two instructions, set by scalar moves, and no mask operand: a lane without the neighbour is
    // not written.  The time loop runs with all 64 lanes (the kernel's only exit is wave-uniform and stands before it), so EXEC goes
    // back to all ones.
#define CUDDH_EL_ADD_FETCHED(NAME, LANES)                                                                                                  \
    __device__ inline void NAME(pair_t &z0, pair_t &z1, pair_t f0, pair_t f1)                                                              \
    {                                                                                                                                      \
        asm volatile("s_mov_b32 exec_lo, " LANES "\n\t"                                                                                    \
                     "s_mov_b32 exec_hi, " LANES "\n\t"                                                                                    \
                     "v_pk_add_f32 %0, %0, %2\n\t"                                                                                         \
                     "v_pk_add_f32 %1, %1, %3\n\t"                                                                                         \
                     "s_mov_b64 exec, -1\n\t"                                                                                              \
                     : "+v"(z0), "+v"(z1)                                                                                                  \
                     : "v"(f0), "v"(f1));                                                                                                  \
    }
    CUDDH_EL_ADD_FETCHED(element_add_from_the_left, "0xeeeeeeee")
    CUDDH_EL_ADD_FETCHED(element_add_from_the_right, "0x77777777")
#undef CUDDH_EL_ADD_FETCHED
    // x of another lane over the LDS pipe: ds_swizzle_b32, which uses no LDS storage and, unlike ds_bpermute_b32, no address
    // register (one source register to move to the LDS, not two).  The pattern is the instruction's offset field:
    // a quad permutation for xi (the four lanes of a quad are ex = 0..3 of one eta-row; a lane without the neighbour reads itself),
    // a rotation by 4 within each 32-lane half for eta (a lane without the neighbour reads another row, or the other end of its own).
    constexpr int FETCH_RIGHT = 0x8000 | 1 | (2 << 2) | (3 << 4) | (3 << 6); // lane + 1
    constexpr int FETCH_LEFT = 0x8000 | 0 | (0 << 2) | (1 << 4) | (2 << 6);  // lane - 1
    constexpr int FETCH_ABOVE = 0xC000 | (0 << 10) | (4 << 5);               // lane + 4, modulo 32
    constexpr int FETCH_BELOW = 0xC000 | (1 << 10) | (4 << 5);               // lane - 4, modulo 32
    template <int PATTERN>
    __device__ inline float lane_fetch(float x)
    {
        return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, x), PATTERN));
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

    // The paired chain with a head: t = head + Dg w in one FMA where element_lane_pair_product<K, H, true> opens with the bare
    // product, every other term at its place in that order.  7 instructions per pair as there; what the head costs is
    // the caller's (wh_march_pairs_scaled).
    template <int K, int H>
    __device__ inline pair_t element_lane_pair_product_headed(const pair_t (&w)[8], const pair_t head, const pair_t (&Bx)[6], const float (&By)[16],
                                                              const pair_t (&Dg)[8])
    {
        constexpr int la = H, lb = 3 - H, P = K + 4 * H, Q = K + 4 * (1 - H);
        pair_t t = pk_fma(Dg[P], w[P], head);
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
    // the pairs of HEADS open their chain on head[P], the others run the paired chain as it is
    template <unsigned HEADS, int K, int H>
    __device__ inline pair_t element_lane_pair_product_select(const pair_t (&w)[8], const pair_t (&head)[8], const pair_t (&Bx)[6], const float (&By)[16],
                                                              const pair_t (&Dg)[8])
    {
        if constexpr (((HEADS >> (K + 4 * H)) & 1u) != 0)
            return element_lane_pair_product_headed<K, H>(w, head[K + 4 * H], Bx, By, Dg);
        else
            return element_lane_pair_product<K, H, true>(w, Bx, By, Dg);
    }
    template <unsigned HEADS>
    __device__ inline void element_lane_products_headed(const pair_t (&w)[8], const pair_t (&head)[8], pair_t (&z)[8], const pair_t (&Bx)[6],
                                                        const float (&By)[16], const pair_t (&Dg)[8])
    {
        z[0] = element_lane_pair_product_select<HEADS, 0, 0>(w, head, Bx, By, Dg);
        z[1] = element_lane_pair_product_select<HEADS, 1, 0>(w, head, Bx, By, Dg);
        z[2] = element_lane_pair_product_select<HEADS, 2, 0>(w, head, Bx, By, Dg);
        z[3] = element_lane_pair_product_select<HEADS, 3, 0>(w, head, Bx, By, Dg);
        z[4] = element_lane_pair_product_select<HEADS, 0, 1>(w, head, Bx, By, Dg);
        z[5] = element_lane_pair_product_select<HEADS, 1, 1>(w, head, Bx, By, Dg);
        z[6] = element_lane_pair_product_select<HEADS, 2, 1>(w, head, Bx, By, Dg);
        z[7] = element_lane_pair_product_select<HEADS, 3, 1>(w, head, Bx, By, Dg);
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

    // wh_march_pairs with the sources in the first WaveHoltz pass only (forcing 2, cuddh_hip_ddh_plan_set_forcing).  A pass is
    // affine in its start value, X' = Pi X + r with X = (u, v), and r, what the sources F and Gf contribute, is the same in
    // every pass; the first pass starts from 0 and returns exactly r.  So the first pass runs wh_march_pairs' loop, expression
    // for expression (with one pass the two are the same instructions on the same values), and parks r; every later pass runs a
    // loop with no source terms at all (dq = z on the interior pairs, -Hi q + z on the others: no F, Gf, cs or sn, the same loop
    // for both LEAN forms) and adds r behind it.  Pi is untouched.  2 packed FMAs per non-interior pair and half step go, 24 of
    // 228 per wavefront-step in the action form and 32 of 244 in the form with x, in all passes but the first; the rounding
    // is new (r is rounded once and added, not summed step by step into every pass).  The first pass stands before the loop
    // over the others and not inside it, so that F, Gf and cs / sn are dead from there on; DM2 is DM for the loop without
    // sources, which has their registers to spare.  r waits in LDS, 16 pairs per lane in slots of the lane's own, [pair][thread]
    // so that the 64-bit accesses of a wavefront do not conflict: 32 KB for the caller's 256 threads, written behind the first
    // time loop and read behind the others, never inside one, and by the lane that wrote it, so no barrier.
    template <int LEAN, unsigned INTERIOR, unsigned DM, unsigned DM2, int N, typename Sweep>
    __device__ inline void wh_march_pairs_once(const DdhArgs<float> &A, const int nt, const float dt, const float *__restrict__ filt,
                                               const float *__restrict__ cs, const float *__restrict__ sn, const pair_t (&invm)[N],
                                               const pair_t (&Hi)[N], const pair_t (&F)[N], const pair_t (&Gf)[N], pair_t (&u)[N], pair_t (&v)[N],
                                               Sweep sweep)
    {
        static_assert(LEAN == 1 || LEAN == 2, "the packed loop has wh_march's LEAN forms only");
        __shared__ pair_t parked[2 * N][256];
        pair_t p[N], q[N], hm[N];
        const float half_dt = 0.5f * dt;
#pragma unroll
        for (int l = 0; l < N; ++l)
        {
            p[l] = q[l] = u[l] = v[l] = 0;
            hm[l] = half_dt * invm[l];
        }
        // one pass from (u, v), with the sources or without; MASK: the pairs with dm
        auto pass = [&](auto SOURCES, auto MASK, const pair_t(&dm)[N])
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
                [[maybe_unused]] float c0, s0, c1, s1;
                if constexpr (SOURCES.value)
                {
                    c0 = cs[2 * it - 2], s0 = sn[2 * it - 2];
                    c1 = cs[2 * it - 1], s1 = sn[2 * it - 1];
                }
                const float kw = filt[it];
                pair_t z[N], ph[N], qh[N];

                sweep(p, z);
#pragma unroll
                for (int l = 0; l < N; ++l)
                {
                    pair_t dq = ((INTERIOR >> l) & 1u) != 0 ? z[l] : pk_fma(-Hi[l], q[l], z[l]);
                    if constexpr (SOURCES.value)
                        if (((INTERIOR >> l) & 1u) == 0 || LEAN == 2)
                            dq = pk_fma(s0, Gf[l], pk_fma(c0, F[l], dq));
                    ph[l] = pk_fma(-half_dt, q[l], p[l]);
                    qh[l] = pk_fma(hm[l], dq, q[l]);
                    p[l] = pk_fma(-dt, qh[l], p[l]);
                }
                sweep(ph, z);
#pragma unroll
                for (int l = 0; l < N; ++l)
                {
                    pair_t dq = ((INTERIOR >> l) & 1u) != 0 ? z[l] : pk_fma(-Hi[l], qh[l], z[l]);
                    if constexpr (SOURCES.value)
                        if (((INTERIOR >> l) & 1u) == 0 || LEAN == 2)
                            dq = pk_fma(s1, Gf[l], pk_fma(c1, F[l], dq));
                    if (((MASK.value >> l) & 1u) != 0)
                        q[l] = pk_fma(dm[l], dq, q[l]);
                    else
                        q[l] = pk_fma(hm[l], 2.0f * dq, q[l]);
                    u[l] = pk_fma(kw, p[l], u[l]);
                    v[l] = pk_fma(kw, q[l], v[l]);
                }
            }
        };
        if (A.wh_iters < 1)
            return;
        pair_t(*const r)[256] = reinterpret_cast<pair_t(*)[256]>(&parked[0][threadIdx.x]);
        {
            pair_t dm[N];
#pragma unroll
            for (int l = 0; l < N; ++l)
                dm[l] = ((DM >> l) & 1u) != 0 ? dt * invm[l] : pair_t{0.0f, 0.0f};
            pass(std::true_type{}, std::integral_constant<unsigned, DM>{}, dm);
        }
        if (A.wh_iters < 2)
            return;
#pragma unroll
        for (int l = 0; l < N; ++l)
        {
            r[l][0] = u[l];
            r[N + l][0] = v[l];
        }
        pair_t dm2[N];
#pragma unroll
        for (int l = 0; l < N; ++l)
            dm2[l] = ((DM2 >> l) & 1u) != 0 ? hm[l] + hm[l] : pair_t{0.0f, 0.0f}; // dt invm exactly: doubling is exact (above)
        for (int whit = 1; whit < A.wh_iters; ++whit)
        {
            pass(std::false_type{}, std::integral_constant<unsigned, DM2>{}, dm2);
#pragma unroll
            for (int l = 0; l < N; ++l)
            {
                u[l] += r[l][0];
                v[l] += r[N + l][0];
            }
        }
    }

    // wh_march_pairs_once with the velocity carried scaled and its midpoint update folded into the sweep (march 2,
    // cuddh_hip_ddh_plan_set_march).  With hm = half_dt invm the midpoint velocity of a non-interior node is
    //     qh = q + hm (z - Hi q),   so   qh / hm = 2 (1 - hm Hi) q / (2 hm) + z.
    // The state is qs = q / (2 hm).  The chain of the first sweep opens on alpha qs, alpha = 2 (1 - hm Hi), where it opened with
    // the bare product Dg w: that product becomes an FMA onto the head and the assembled result IS qt = qh / hm; wh_march_pairs'
    // two instructions dq = -Hi q + z and qh = q + hm dq are gone.  With c = dt hm and b = hm Hi the step is
    //     qt = assemble(alpha / m qs + chain(p)),   ph = p - c qs,   p -= c qt,
    //     z  = assemble(-b / m qt + chain(ph)),     qs += z,         u += kw p,   vs += kw qs,
    // 8 + 2 packed instructions per pair in the first half step where there were 7 + 4, 8 + 3 in the second as before (the
    // interior pairs, Hi = 0: qs + qs for the first head, no second head).  The assembly sums the chains of all m copies of a
    // shared node (m = 1, 2 or 4, element_lane_inverse_multiplicity), so what enters a head enters it as 1 / m of its value in
    // every copy; division by 2 or 4 is exact and the copies hold the same qs, so they stay bitwise equal.  The sources of the
    // first pass ride on the heads the same way, F / m and Gf / m.
    // The last addition, qs += z, stays an addition onto the state and is NOT folded into the chain as a third head: a chain
    // rounds seven times at the magnitude of its accumulator.  qt is only ever multiplied by c or b, both O(dt), so those
    // roundings do there what the roundings of z do today; qs is the integrated state, and carrying it through a chain would
    // round it seven times per step at its own magnitude.
    // qs and vs = sum kw qs are never converted inside the march: the first pass starts from 0, every later pass starts from vs
    // as it stands, r is parked scaled, and v = vs c (2 / dt) = 2 hm vs once at the end.  No division anywhere, so a node with
    // invm = 0 (c = 0) ends with v = 0 as it does in wh_march_pairs.  Registers per pair: c, alpha / m, -b / m where
    // wh_march_pairs_once keeps hm, Hi, dm.
    template <int LEAN, unsigned INTERIOR, int N, typename SweepHeaded>
    __device__ inline void wh_march_pairs_scaled(const DdhArgs<float> &A, const int nt, const float dt, const float *__restrict__ filt,
                                                 const float *__restrict__ cs, const float *__restrict__ sn, const pair_t (&invm)[N],
                                                 const pair_t (&Hi)[N], const pair_t (&F)[N], const pair_t (&Gf)[N], const pair_t (&rm)[N],
                                                 pair_t (&u)[N], pair_t (&v)[N], SweepHeaded sweep)
    {
        static_assert(LEAN == 1 || LEAN == 2, "the packed loop has wh_march's LEAN forms only");
        constexpr unsigned ALL = (1u << N) - 1u;
        __shared__ pair_t parked[2 * N][256];
        pair_t p[N], q[N], c[N], am[N], bm[N]; // q: qs; am = alpha / m, bm = -b / m
        const float half_dt = 0.5f * dt;
#pragma unroll
        for (int l = 0; l < N; ++l)
        {
            const pair_t hm = half_dt * invm[l], b = hm * Hi[l];
            p[l] = q[l] = u[l] = v[l] = 0;
            c[l] = dt * hm;
            am[l] = (2.0f * (1.0f - b)) * rm[l];
            bm[l] = -b * rm[l];
        }
        // one pass from (u, vs), with the sources or without
        auto pass = [&](auto SOURCES, const pair_t(&Fm)[N], const pair_t(&Gm)[N])
        {
            constexpr bool INNER_SOURCES = SOURCES.value && LEAN == 2; // the form with x has sources on the interior pairs too
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
                [[maybe_unused]] float c0, s0, c1, s1;
                if constexpr (SOURCES.value)
                {
                    c0 = cs[2 * it - 2], s0 = sn[2 * it - 2];
                    c1 = cs[2 * it - 1], s1 = sn[2 * it - 1];
                }
                const float kw = filt[it];
                pair_t z[N], ph[N], qt[N], head[N];

#pragma unroll
                for (int l = 0; l < N; ++l)
                {
                    const bool inner = ((INTERIOR >> l) & 1u) != 0;
                    head[l] = inner ? q[l] + q[l] : am[l] * q[l];
                    if (SOURCES.value && (!inner || LEAN == 2))
                        head[l] = pk_fma(s0, Gm[l], pk_fma(c0, Fm[l], head[l]));
                }
                // ph before the sweep, not beside the update of p behind it: with it there the allocator moves two pairs of qt
                // round the assembly statements, eight v_mov_b32 per step in the loop without sources (profiles/r31)
#pragma unroll
                for (int l = 0; l < N; ++l)
                    ph[l] = pk_fma(-c[l], q[l], p[l]);
                sweep(std::integral_constant<unsigned, ALL>{}, p, head, qt);
#pragma unroll
                for (int l = 0; l < N; ++l)
                    p[l] = pk_fma(-c[l], qt[l], p[l]);
#pragma unroll
                for (int l = 0; l < N; ++l)
                {
                    const bool inner = ((INTERIOR >> l) & 1u) != 0;
                    if (!inner)
                    {
                        head[l] = bm[l] * qt[l];
                        if (SOURCES.value)
                            head[l] = pk_fma(s1, Gm[l], pk_fma(c1, Fm[l], head[l]));
                    }
                    else if (INNER_SOURCES)
                        head[l] = pk_fma(s1, Gm[l], c1 * Fm[l]);
                }
                sweep(std::integral_constant<unsigned, INNER_SOURCES ? ALL : (ALL & ~INTERIOR)>{}, ph, head, z);
#pragma unroll
                for (int l = 0; l < N; ++l)
                {
                    q[l] += z[l]; // onto the state, not through the chain (above)
                    u[l] = pk_fma(kw, p[l], u[l]);
                    v[l] = pk_fma(kw, q[l], v[l]);
                }
            }
        };
        if (A.wh_iters < 1)
            return;
        pair_t(*const r)[256] = reinterpret_cast<pair_t(*)[256]>(&parked[0][threadIdx.x]);
        {
            pair_t Fm[N], Gm[N];
#pragma unroll
            for (int l = 0; l < N; ++l)
            {
                Fm[l] = F[l] * rm[l];
                Gm[l] = Gf[l] * rm[l];
            }
            pass(std::true_type{}, Fm, Gm);
        }
        if (A.wh_iters >= 2)
        {
#pragma unroll
            for (int l = 0; l < N; ++l)
            {
                r[l][0] = u[l];
                r[N + l][0] = v[l];
            }
            for (int whit = 1; whit < A.wh_iters; ++whit)
            {
                pass(std::false_type{}, F, Gf); // F and Gf are not read
#pragma unroll
                for (int l = 0; l < N; ++l)
                {
                    u[l] += r[l][0];
                    v[l] += r[N + l][0];
                }
            }
        }
        const float two_over_dt = 2.0f / dt;
#pragma unroll
        for (int l = 0; l < N; ++l)
            v[l] *= c[l] * two_over_dt;
    }

    // wh_march_pairs_scaled with the state carried already multiplied by its chain head (head 2, cuddh_hip_ddh_plan_set_head).
    // What opens the first sweep's chain there, am qs (am = alpha / m), is only ever the start of an FMA chain, so the state is
    // Y = am qs (the same float in all m copies of a node, since am is) and the chain opens as fma(Dg, p, Y): no head
    // instruction.  With c2 = c / am the step is
    //     ph = p - c2 Y,   qt = assemble(Y + chain(p)),    p -= c qt,
    //     z  = assemble(bm qt + chain(ph)),   Y = fma(am, z, Y),   u += kw p,   vy += kw Y,
    // 20 packed instructions per non-interior pair and step where wh_march_pairs_scaled has 21.  Y = fma(am, z, Y) is one
    // rounding onto the integrated state, as qs += z is there, and not a third chain head (above).  The interior pairs carry
    // Y = 2 qs (am = 2, c2 = c / 2, Y += 2 z): every operation on them is the one of wh_march_pairs_scaled on a doubled value,
    // so their bits are those of that march and its qs + qs goes too.  vy and the parked r stay in the unit of Y across the
    // passes; v = vy c2 (2 / dt) once at the end.  c2 is formed once per launch, before the first pass: am = 2 (1 - hm Hi) / m
    // is not 0 in a stable solve, and invm = 0 gives c = 0, c2 = 0 and v = 0.  The sources of the first pass ride on Y as they
    // ride on the head there.
    // Registers: four coefficients per non-interior pair (c, c2, am, bm) where wh_march_pairs_scaled has three, twelve registers
    // more on a loop that stood at 164 of the 168 that three wavefronts per SIMD leave.  So bm waits in LDS beside r,
    // [pair][thread] in slots of the lane's own (six pairs: 12 KB, 44 KB a workgroup, 132 of 160 KB for three workgroups per CU),
    // and is read once per step by the lane that wrote it, so no barrier: three ds_read2st64_b64 per step, the first LDS accesses
    // in a time loop of this family.  The first time loop, which has the sources F / m and Gf / m in registers, reads c2 the same
    // way, from the slots in which r waits behind it, and c2 comes back into registers before r is parked.
    // Vector instructions per wavefront-step, first / later passes (profiles/r32): action form 214 / 190 where
    // wh_march_pairs_scaled has 226 / 198, no v_mov_b32 in either loop, 167 VGPRs, no scratch.
    template <int LEAN, unsigned INTERIOR, bool FETCHED = false, int N, typename SweepHeaded>
    __device__ inline void wh_march_pairs_carried(const DdhArgs<float> &A, const int nt, const float dt, const float *__restrict__ filt,
                                                  const float *__restrict__ cs, const float *__restrict__ sn, const pair_t (&invm)[N],
                                                  const pair_t (&Hi)[N], const pair_t (&F)[N], const pair_t (&Gf)[N], const pair_t (&rm)[N],
                                                  pair_t (&u)[N], pair_t (&v)[N], SweepHeaded sweep)
    {
        static_assert(LEAN == 1 || LEAN == 2, "the packed loop has wh_march's LEAN forms only");
        constexpr unsigned ALL = (1u << N) - 1u;
        // what fits three wavefronts per SIMD without scratch: the action form carries the interior pairs too and asks for bm at
        // the top of the step; the form with x, which has sources on the interior pairs, leaves those as they are (the same bits)
        // and asks for bm behind the first sweep (profiles/r32)
        constexpr bool CARRY_INNER = LEAN == 1;
        constexpr int BM_WHERE = LEAN == 1 ? 0 : 1;
        __shared__ pair_t parked[2 * N][256];
        pair_t p[N], q[N], c[N], c2[N], am[N], bm[N]; // q: Y; am = alpha / m, bm = -b / m, c2 = c / am
        const float half_dt = 0.5f * dt;
        constexpr int NO = N - __builtin_popcount(INTERIOR); // the non-interior pairs, and a pair's place among them
        auto slot = [](int l) { return __builtin_popcount(~INTERIOR & ((1u << l) - 1u)); };
        // bm in slots of its own; c2 through the first pass in the slots where r waits behind it (the first time loop has the
        // sources in the registers c2 has in the others)
        __shared__ pair_t parked_bm[NO][256];
        lds_pair_t *coef = (lds_pair_t *)&parked_bm[0][threadIdx.x], *coef2 = (lds_pair_t *)&parked[0][threadIdx.x];
        // a read the compiler cannot move out of the time loop, into the registers it is there to spare: the address passes through
        // an empty statement first, in place (a copy would cost a v_mov_b32 per step).  Plain LDS reads otherwise, with immediate
        // offsets, scheduled and waited for by the compiler
        auto coef_now = [](lds_pair_t *&here)
        {
            asm volatile("" : "+v"(here));
            return here;
        };
#pragma unroll
        for (int l = 0; l < N; ++l)
        {
            const bool inner = ((INTERIOR >> l) & 1u) != 0;
            const pair_t hm = half_dt * invm[l], b = hm * Hi[l];
            p[l] = q[l] = u[l] = v[l] = 0;
            c[l] = dt * hm;
            am[l] = inner ? pair_t{2.0f, 2.0f} : (2.0f * (1.0f - b)) * rm[l];
            c2[l] = inner ? (CARRY_INNER ? 0.5f * c[l] : c[l]) : c[l] / am[l];
            bm[l] = -b * rm[l];
            if (!inner)
            {
                coef[256 * slot(l)] = bm[l];
                coef2[256 * slot(l)] = c2[l];
                if constexpr (FETCHED) // and am behind c2: the first time loop has the fetched halves in its place
                    coef2[256 * (NO + slot(l))] = am[l];
            }
        }
        // one pass from (u, vy), with the sources or without
        auto pass = [&](auto SOURCES, const pair_t(&Fm)[N], const pair_t(&Gm)[N])
        {
            constexpr bool INNER_SOURCES = SOURCES.value && LEAN == 2; // the form with x has sources on the interior pairs too
            // FETCHED: the fetched halves wait in registers while the other chains run, and the first sweep of the loop with the
            // sources has none for bm beside them
            constexpr int BM_HERE = FETCHED && SOURCES.value ? 1 : BM_WHERE;
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
                [[maybe_unused]] float c0, s0, c1, s1;
                if constexpr (SOURCES.value)
                {
                    c0 = cs[2 * it - 2], s0 = sn[2 * it - 2];
                    c1 = cs[2 * it - 1], s1 = sn[2 * it - 1];
                }
                const float kw = filt[it];
                pair_t z[N], ph[N], qt[N], head[N], bl[N], cl[N];
                lds_pair_t *const here = coef_now(coef);
                [[maybe_unused]] lds_pair_t *here2 = nullptr;
                if constexpr (SOURCES.value)
                    here2 = coef_now(coef2);

#pragma unroll
                for (int l = 0; l < N; ++l)
                    cl[l] = SOURCES.value && ((INTERIOR >> l) & 1u) == 0 ? here2[256 * slot(l)] : c2[l];
                if constexpr (BM_HERE == 0)
                {
#pragma unroll
                    for (int l = 0; l < N; ++l)
                        if (((INTERIOR >> l) & 1u) == 0)
                            bl[l] = here[256 * slot(l)];
                }
#pragma unroll
                for (int l = 0; l < N; ++l)
                {
                    const bool inner = ((INTERIOR >> l) & 1u) != 0;
                    head[l] = inner && !CARRY_INNER ? q[l] + q[l] : q[l];
                    if (SOURCES.value && (!inner || LEAN == 2))
                        head[l] = pk_fma(s0, Gm[l], pk_fma(c0, Fm[l], head[l]));
                }
                // ph before the sweep, as in wh_march_pairs_scaled
#pragma unroll
                for (int l = 0; l < N; ++l)
                    ph[l] = pk_fma(-cl[l], q[l], p[l]);
                sweep(std::integral_constant<unsigned, ALL>{}, p, head, qt);
                if constexpr (BM_HERE == 1)
                {
#pragma unroll
                    for (int l = 0; l < N; ++l)
                        if (((INTERIOR >> l) & 1u) == 0)
                            bl[l] = here[256 * slot(l)];
                }
#pragma unroll
                for (int l = 0; l < N; ++l)
                    p[l] = pk_fma(-c[l], qt[l], p[l]);
#pragma unroll
                for (int l = 0; l < N; ++l)
                {
                    const bool inner = ((INTERIOR >> l) & 1u) != 0;
                    if (!inner)
                    {
                        head[l] = bl[l] * qt[l];
                        if (SOURCES.value)
                            head[l] = pk_fma(s1, Gm[l], pk_fma(c1, Fm[l], head[l]));
                    }
                    else if (INNER_SOURCES)
                        head[l] = pk_fma(s1, Gm[l], c1 * Fm[l]);
                }
                sweep(std::integral_constant<unsigned, INNER_SOURCES ? ALL : (ALL & ~INTERIOR)>{}, ph, head, z);
                [[maybe_unused]] lds_pair_t *here3 = nullptr;
                if constexpr (SOURCES.value && FETCHED)
                    here3 = coef_now(coef2); // behind the second sweep's additions: am is asked for where it is needed
#pragma unroll
                for (int l = 0; l < N; ++l)
                {
                    const bool inner = ((INTERIOR >> l) & 1u) != 0;
                    const pair_t al = SOURCES.value && FETCHED && !inner ? pair_t(here3[256 * (NO + slot(l))]) : am[l];
                    q[l] = inner ? (CARRY_INNER ? pk_fma(2.0f, z[l], q[l]) : q[l] + z[l]) : pk_fma(al, z[l], q[l]); // onto the state, one rounding (above)
                    u[l] = pk_fma(kw, p[l], u[l]);
                    v[l] = pk_fma(kw, q[l], v[l]);
                }
            }
        };
        if (A.wh_iters < 1)
            return;
        pair_t(*const r)[256] = reinterpret_cast<pair_t(*)[256]>(&parked[0][threadIdx.x]);
        {
            // the sources ride on Y = am qs: in its unit, F / m and Gf / m of wh_march_pairs_scaled's heads as they are
            pair_t Fm[N], Gm[N];
#pragma unroll
            for (int l = 0; l < N; ++l)
            {
                Fm[l] = F[l] * rm[l];
                Gm[l] = Gf[l] * rm[l];
            }
            pass(std::true_type{}, Fm, Gm);
        }
        {
            // c2 comes back into registers behind the first time loop, which has the sources in its place
            lds_pair_t *here = coef_now(coef2);
#pragma unroll
            for (int l = 0; l < N; ++l)
                if (((INTERIOR >> l) & 1u) == 0)
                {
                    c2[l] = here[256 * slot(l)];
                    if constexpr (FETCHED)
                        am[l] = here[256 * (NO + slot(l))];
                }
        }
        if (A.wh_iters >= 2)
        {
#pragma unroll
            for (int l = 0; l < N; ++l)
            {
                r[l][0] = u[l];
                r[N + l][0] = v[l];
            }
            for (int whit = 1; whit < A.wh_iters; ++whit)
            {
                pass(std::false_type{}, F, Gf); // F and Gf are not read
#pragma unroll
                for (int l = 0; l < N; ++l)
                {
                    u[l] += r[l][0];
                    v[l] += r[N + l][0];
                }
            }
        }
        const float two_over_dt = 2.0f / dt;
#pragma unroll
        for (int l = 0; l < N; ++l)
            v[l] *= c2[l] * two_over_dt;
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

    // ---------------------------------------------------------------- the row-per-subdomain kernel (kernels 5, 12 and 13)
    // Kernel 5's element-lane form (NB = 4) and kernel 12 (NB = 5), both documented above, and kernel 13 for either.
    // The frame is written once, in the kernel body and not behind a function of its own: a body moved unchanged into a
    // __device__ __forceinline__ template compiled to other code in all sixteen instantiations tried (the callee is optimised
    // before it is inlined).  What depends on NB is constants, the state's type, and the `if constexpr (NB == 4)` branches.
    // NB: nodes per element side, 4 (the state in pairs, wh_march_pairs) or 5 (a register per node, wh_march).
    // FETCHED: CARRIED with the neighbour sums fetched both ways over the LDS pipe (assembly 2), the same bits
    // FORCED, HOLD: as in ddh_mfma_kernel.  LAST_COPY: the owner rule turned round.
    // PAIRED: the paired chains in the sweep (element_lane_pair_product), NB = 4 and the one-grid kernel only
    // ONCE: the sources in the first WaveHoltz pass only (wh_march_pairs_once; forcing 2), with PAIRED only.  The only
    //     instantiations that take LDS (32 KB a workgroup, three workgroups per CU: 96 KB of 160)
    // SCALED: ONCE with the velocity carried scaled and its midpoint update folded into the sweep (wh_march_pairs_scaled; march 2)
    // CARRIED: SCALED with the velocity carried already multiplied by the head coefficient of the first sweep's chain
    //     (wh_march_pairs_carried; head 2)
    // Grids: nothing, or the plan's TimeGrids (kernel 13: a pass per distinct grid among the four rows, GroupedRows; RK2 only)
    // Sep: [Bx | By | Dg | W | 1 / W], NB NB floats each (build_element_lane_tables).
    // A stays the FIRST parameter: reread_args reads it at offset 0 of the kernel-argument segment.
    // Wavefronts per SIMD: three at NB = 4; at NB = 5 two, and one in the form with x.
    template <int NB, bool FORCED, bool HOLD, bool LAST_COPY, bool PAIRED, bool ONCE, bool SCALED, bool CARRIED, bool FETCHED, typename... Grids>
    __global__ void __launch_bounds__(256, NB == 4 ? 3 : (FORCED ? 1 : 2))
        ddh_element_lane_kernel(DdhArgs<float> A, const float *__restrict__ Sep, const float *__restrict__ filt, const float *__restrict__ cs,
                                const float *__restrict__ sn, Grids... grids)
    {
        constexpr bool GROUPED = sizeof...(Grids) > 0;
        constexpr int NN = NB * NB;           // nodes per element, and per lane
        constexpr int NS = NB == 4 ? 8 : NN;  // state values per lane: pairs of nodes (el_pair, el_half) or nodes
        using state_t = std::conditional_t<NB == 4, pair_t, float>;
        static_assert(NB == 4 || NB == 5, "the assembly statements exist for 4 and 5 values a side");
        static_assert(sizeof...(Grids) <= 1 && scheme_of<Grids...> == 0, "one grid, or TimeGrids; no RK4 form");
        static_assert(!(PAIRED && NB != 4), "the paired chains are those of the packed form");
        static_assert(!(PAIRED && sizeof...(Grids) > 0), "the paired chains are built for the one-grid kernel only");
        static_assert(!(ONCE && !PAIRED), "the march with the sources in the first pass only is built beside the paired chains only");
        static_assert(!(SCALED && !ONCE), "the scaled march is built with the sources in the first pass only");
        static_assert(!(CARRIED && !SCALED), "the carried head is built on the scaled march only");
        static_assert(!(FETCHED && !CARRIED), "the assembly over the LDS pipe is built on the carried head only");
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
            sI = Ar.sI + 16 * NN * (size_t)s + NN * (tid & 15);
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

        state_t invm[NS], Hi[NS], F[NS], Gf[NS], u[NS], v[NS];
#pragma unroll
        for (int n = 0; n < NN; ++n)
        {
            if constexpr (NB == 4)
            {
                const int P = el_pair(n & 3, n >> 2), half = el_half(n >> 2);
                float im, hi, f, gf;
                load_dof(Ar, s, sI[n], fdof, im, hi, f, gf);
                fold_weight(Sep[3 * NN + n + again], Sep[4 * NN + n + again], im, hi, f, gf);
                invm[P][half] = im, Hi[P][half] = hi, F[P][half] = f, Gf[P][half] = gf;
            }
            else
            {
                // straight into the registers: through locals, as above, the forms with x order the last products otherwise
                load_dof(Ar, s, sI[n], fdof, invm[n], Hi[n], F[n], Gf[n]);
                fold_weight(Sep[3 * NN + n + again], Sep[4 * NN + n + again], invm[n], Hi[n], F[n], Gf[n]);
            }
        }
        // wave-uniform: scalar registers for the whole time loop.  Bx(k, j) at k + NB j, By(l, j) at l + NB j, Dg(k, l) at
        // k + NB l; NB == 4: Dg in the pairs of the state, of Bx the off-diagonals, two to a pair (bx_slot)
        float By[NN];
        state_t Bx[NB == 4 ? 6 : NN], Dg[NS];
#pragma unroll
        for (int i = 0; i < NN; ++i)
        {
            if constexpr (NB == 4)
            {
                if ((i & 3) != (i >> 2))
                    Bx[bx_slot(i & 3, i >> 2) / 2][bx_slot(i & 3, i >> 2) % 2] = Sep[i];
                By[i] = Sep[NN + i];
                Dg[el_pair(i & 3, i >> 2)][el_half(i >> 2)] = Sep[2 * NN + i];
            }
            else
            {
                Bx[i] = Sep[i];
                By[i] = Sep[NN + i];
                Dg[i] = Sep[2 * NN + i];
            }
        }
        const float mR = (threadIdx.x & 3) < 3 ? 1.0f : 0.0f; // ex < 3: the only mask left, for the xi sums

        // in-lane products, then the assembly: xi neighbours first (my k == NB - 1 column meets the k == 0 column of lane + 1),
        // eta neighbours on the xi-assembled values (my l == NB - 1 row meets the l == 0 row of lane + 4)
        auto sweep = [&](const state_t(&w)[NS], state_t(&z)[NS])
        {
            if constexpr (NB == 4)
            {
                element_lane_products_packed<PAIRED>(w, z, Bx, By, Dg);
                // the 32-bit halves of the pairs
                float hi[4] = {z[3].x, z[7].x, z[7].y, z[3].y}, lo[4] = {z[0].x, z[4].x, z[4].y, z[0].y}; // l = 0, 1, 2, 3
                element_assemble_xi_row_asm(hi, lo, mR);
                z[3].x = hi[0], z[7].x = hi[1], z[7].y = hi[2], z[3].y = hi[3];
                z[0].x = lo[0], z[4].x = lo[1], z[4].y = lo[2], z[0].y = lo[3];
                float up[4] = {z[0].y, z[1].y, z[2].y, z[3].y}, dn[4] = {z[0].x, z[1].x, z[2].x, z[3].x};
                element_assemble_eta_row_asm(up, dn);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                {
                    z[k].y = up[k];
                    z[k].x = dn[k];
                }
            }
            else
            {
                element_lane_products<5>(w, z, Bx, By, Dg);
                float hi[5] = {z[4], z[9], z[14], z[19], z[24]}, lo[5] = {z[0], z[5], z[10], z[15], z[20]};
                element_assemble_xi_row5_asm(hi, lo, mR);
#pragma unroll
                for (int l = 0; l < 5; ++l)
                {
                    z[4 + 5 * l] = hi[l];
                    z[0 + 5 * l] = lo[l];
                }
                float up[5] = {z[20], z[21], z[22], z[23], z[24]}, dn[5] = {z[0], z[1], z[2], z[3], z[4]};
                element_assemble_eta_row5_asm(up, dn);
#pragma unroll
                for (int k = 0; k < 5; ++k)
                {
                    z[k + 20] = up[k];
                    z[k] = dn[k];
                }
            }
        };
        if constexpr (NB == 4 && SCALED)
        {
            // the chains of the pairs in HEADS open on head[P]; the assembly is sweep's
            // FETCHED: the eta masks as the pair the state's pairs need: (ey > 0, ey < 3)
            [[maybe_unused]] const pair_t my = {(threadIdx.x & 12) > 0 ? 1.0f : 0.0f, (threadIdx.x & 12) < 12 ? 1.0f : 0.0f};
            auto sweep_headed = [&](auto HEADS, const pair_t(&w)[8], const pair_t(&head)[8], pair_t(&z)[8])
            {
                if constexpr (FETCHED)
                {
                    // Assembly 2: every copy of a shared node fetches the other copy's partial sum and adds it itself, a + b in
                    // one lane and b + a in the other: the same float.  A lane without that neighbour does not add what it
                    // fetched (xi) or multiplies it by 0 (eta).  The pairs the xi fetches read come first, and the other chains stand behind
                    // the fetches: the round trip over the LDS pipe hides behind them.
                    constexpr unsigned H = HEADS.value;
                    constexpr int RIGHT = FETCH_RIGHT, LEFT = FETCH_LEFT, ABOVE = FETCH_ABOVE, BELOW = FETCH_BELOW;
                    z[0] = element_lane_pair_product_select<H, 0, 0>(w, head, Bx, By, Dg);
                    z[3] = element_lane_pair_product_select<H, 3, 0>(w, head, Bx, By, Dg);
                    z[4] = element_lane_pair_product_select<H, 0, 1>(w, head, Bx, By, Dg);
                    z[7] = element_lane_pair_product_select<H, 3, 1>(w, head, Bx, By, Dg);
                    // xi: my k == 0 column takes the k == 3 column of lane - 1, my k == 3 column the k == 0 column of lane + 1
                    const pair_t f0 = {lane_fetch<LEFT>(z[3].x), lane_fetch<LEFT>(z[3].y)};
                    const pair_t f4 = {lane_fetch<LEFT>(z[7].x), lane_fetch<LEFT>(z[7].y)};
                    const pair_t f3 = {lane_fetch<RIGHT>(z[0].x), lane_fetch<RIGHT>(z[0].y)};
                    const pair_t f7 = {lane_fetch<RIGHT>(z[4].x), lane_fetch<RIGHT>(z[4].y)};
                    // nothing crosses this line: left alone, the scheduler runs all eight chains first and waits for the xi fetches
                    // where it issued them.  One line only: with more of them (behind the eta fetches of the pairs 1 and 2, before
                    // the xi additions) the allocator copies pairs of the state round the statements, 40 to 72 v_mov_b64 a step
                    // (profiles/r33)
                    __builtin_amdgcn_sched_barrier(0);
                    z[1] = element_lane_pair_product_select<H, 1, 0>(w, head, Bx, By, Dg);
                    z[2] = element_lane_pair_product_select<H, 2, 0>(w, head, Bx, By, Dg);
                    // eta: my l == 0 row (.x) takes the l == 3 row (.y) of lane - 4, my l == 3 row the l == 0 row of lane + 4;
                    // the pairs 1 and 2 have no part in xi
                    const pair_t g1 = {lane_fetch<BELOW>(z[1].y), lane_fetch<ABOVE>(z[1].x)};
                    const pair_t g2 = {lane_fetch<BELOW>(z[2].y), lane_fetch<ABOVE>(z[2].x)};
                    z[5] = element_lane_pair_product_select<H, 1, 1>(w, head, Bx, By, Dg);
                    z[6] = element_lane_pair_product_select<H, 2, 1>(w, head, Bx, By, Dg);
                    element_add_from_the_left(z[0], z[4], f0, f4);
                    element_add_from_the_right(z[3], z[7], f3, f7);
                    // the corners: eta on the xi results
                    const pair_t g0 = {lane_fetch<BELOW>(z[0].y), lane_fetch<ABOVE>(z[0].x)};
                    const pair_t g3 = {lane_fetch<BELOW>(z[3].y), lane_fetch<ABOVE>(z[3].x)};
                    z[1] = pk_fma(my, g1, z[1]);
                    z[2] = pk_fma(my, g2, z[2]);
                    z[0] = pk_fma(my, g0, z[0]);
                    z[3] = pk_fma(my, g3, z[3]);
                    return;
                }
                element_lane_products_headed<HEADS.value>(w, head, z, Bx, By, Dg);
                float hi[4] = {z[3].x, z[7].x, z[7].y, z[3].y}, lo[4] = {z[0].x, z[4].x, z[4].y, z[0].y}; // l = 0, 1, 2, 3
                element_assemble_xi_row_asm(hi, lo, mR);
                z[3].x = hi[0], z[7].x = hi[1], z[7].y = hi[2], z[3].y = hi[3];
                z[0].x = lo[0], z[4].x = lo[1], z[4].y = lo[2], z[0].y = lo[3];
                // k = 0, 3, 1, 2: the order of the four independent sums is free, and in this one the first time loop of the
                // action form keeps two copies fewer (profiles/r31)
                float up[4] = {z[0].y, z[3].y, z[1].y, z[2].y}, dn[4] = {z[0].x, z[3].x, z[1].x, z[2].x};
                element_assemble_eta_row_asm(up, dn);
                z[0].y = up[0], z[3].y = up[1], z[1].y = up[2], z[2].y = up[3];
                z[0].x = dn[0], z[3].x = dn[1], z[1].x = dn[2], z[2].x = dn[3];
            };
            pair_t rm[8];
#pragma unroll
            for (int n = 0; n < 16; ++n)
                rm[el_pair(n & 3, n >> 2)][el_half(n >> 2)] = element_lane_inverse_multiplicity<4, 4>(n, threadIdx.x);
            if constexpr (CARRIED)
                wh_march_pairs_carried<FORCED ? 2 : 1, ELEMENT_INTERIOR_PAIRS, FETCHED>(Ar, tg.nt, tg.dt, tg.filt, tg.cs, tg.sn, invm, Hi, F, Gf, rm, u, v,
                                                                                                  sweep_headed);
            else
                wh_march_pairs_scaled<FORCED ? 2 : 1, ELEMENT_INTERIOR_PAIRS>(Ar, tg.nt, tg.dt, tg.filt, tg.cs, tg.sn, invm, Hi, F, Gf, rm, u, v, sweep_headed);
        }
        else if constexpr (NB == 4 && ONCE)
            wh_march_pairs_once<FORCED ? 2 : 1, ELEMENT_INTERIOR_PAIRS, ELEMENT_LANE_ONCE_FIRST_DM_PAIRS(FORCED), ELEMENT_LANE_ONCE_DM_PAIRS>(
                Ar, tg.nt, tg.dt, tg.filt, tg.cs, tg.sn, invm, Hi, F, Gf, u, v, sweep);
        else if constexpr (NB == 4)
            wh_march_pairs<FORCED ? 2 : 1, ELEMENT_INTERIOR_PAIRS, PAIRED ? ELEMENT_LANE_PAIRED_DM_PAIRS(FORCED) : ELEMENT_LANE_DM_PAIRS(FORCED)>(
                Ar, tg.nt, tg.dt, tg.filt, tg.cs, tg.sn, invm, Hi, F, Gf, u, v, sweep);
        else
            wh_march<FORCED ? 2 : 1, element_interior_registers(NB)>(Ar, tg.nt, tg.dt, tg.filt, tg.cs, tg.sn, invm, Hi, F, Gf, u, v, sweep);

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
        for (int n = 0; n < NN; ++n)
        {
            const bool owner = element_lane_owner<NB, 4, LAST_COPY>(n, tid) && (!GROUPED || valid);
            if (owner)
            {
                if constexpr (NB == 4)
                    publish_dof(Ar, s, sI[n], fdof, u[el_pair(n & 3, n >> 2)][el_half(n >> 2)], v[el_pair(n & 3, n >> 2)][el_half(n >> 2)], false);
                else
                    publish_dof(Ar, s, sI[n], fdof, u[n], v[n], false);
            }
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
            fold_weight(Sep4[48 + n], Sep4[64 + n], invm[n], Hi[n], F[n], Gf[n]);
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
            element_lane_products<4>(w, z, Bx, By, Dg);
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
        wh_march<FORCED ? 2 : 1, element_interior_registers(4)>(A, tg.nt, tg.dt, tg.filt, tg.cs, tg.sn, invm, Hi, F, Gf, u, v, sweep);

        // located a second time from a lane index the compiler cannot connect with the first, as in ddh_element_lane_kernel
        // (with time grids the same for the subdomain in its scalar register: nothing derived from it waits through the loop)
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        if constexpr (sizeof...(Grids) > 0)
            asm volatile("" : "+s"(s_wave));
        locate(tid, s, fdof, sI);
#pragma unroll
        for (int n = 0; n < 16; ++n)
            if (element_lane_owner<4, 8, LAST_COPY>(n, tid))
                publish_dof(A, s, sI[n], fdof, u[n], v[n], false);
    }
} // namespace

#endif
