// Tables of the separable DDH sweeps (ddh.hip: kernel 7, the element-lane kernels 5, 11 and 12), from the differentiation
// matrix D and the metric tensor of ONE element.  Host-only double arithmetic (src/element_lane_tables.cpp, no HIP): plan
// creation downloads D and G and uploads the result as it is, and tests read the element-lane table through
// cuddh_element_lane_tables (include/cuddh_hip.h) without a GPU.  DESIGN.md 4.3.
#pragma once

namespace cuddh_k
{
    // The separable sweep's factors, in double, from hD (NB, NB) and the metric hG (3, NB, NB) of an element: needs the metric
    // diagonal (gy == 0) and a product of 1-D factors, gx(k,l) = alpha_k beta_l, gz(k,l) = gamma_k delta_l (rectangles).
    // Ax = D^T diag(alpha) D, Ay = D^T diag(delta) D.  Returns 0 on success, -1 when the geometry does not qualify.
    template <int NB>
    int separable_factors(const float *hD, const float *hG, double (&Ax)[NB][NB], double (&Ay)[NB][NB], double (&beta)[NB], double (&gamma)[NB]);

    // The element-lane table [Bx(k,j) at k + NB j | By(l,j) at l + NB j | Dg(k,l) at k + NB l | W | 1 / W], 5 NB^2 floats: the
    // checks of separable_factors, and that the node weight W(k,l) = gamma_k beta_l is positive and the same on both sides
    // of every shared edge, W(NB-1,l) = W(0,l) and W(k,NB-1) = W(k,0).  W and 1 / W take the weight of the copy with index 0
    // in place of NB - 1, so the copies of a dof scale by one and the same float.  Returns 0 on success, -1 when the
    // geometry does not qualify (out is then not written).  NB = 4 (kernels 5 and 11) and 5 (kernel 12).
    template <int NB>
    int element_lane_tables(const float *hD, const float *hG, float *out);
} // namespace cuddh_k
