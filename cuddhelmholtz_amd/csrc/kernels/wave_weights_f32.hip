// The sweeps of wave_weights.hip (a lattice whose cells each carry a stiffness weight) with state, stencil, weights and
// stages stored and computed in fp32: the stencil and the evaluation order stated at the head of wave_weights.hip, every product-sum
// a fused multiply-add (__builtin_fmaf), `weight` nx ny floats (the caller rounds them once), (K p)(I, J) = +0 where all four
// weights are zero.  The description is the fp64 one, rounded as wave_lattice_f32.hip rounds it (wave::describe; cx, cy and every
// scalar of the call once).  Results depend on (I, J) only: bitwise reproducible; with weights in {0, 1} the bits of wave_cells_f32.hip.
//
// Layout, decomposition (a tile of 128 x 16 nodes, a lane four neighbouring columns, 16-byte LDS pieces), streams, workgroup
// renumbering and the n_basis instantiations are wave_lattice_f32.hip's.  A tile first stages the weights of the cells that contain
// one of its nodes in LDS; when all of them are zero the workgroup returns: it loads and stores no vector.
// The host side below is the family's launcher only (description, extra argument, grid, compile-time n_basis list); the stage
// arguments and their refusals, the dispatch and the six wirings of the entry points are wave_sweep_launch.hpp's.
#include "wave_lattice_common.hpp"
#include "wave_sweep_launch.hpp"

#include "cuddh_hip.h"

using namespace cuddh_k;
using namespace cuddh_k::wave;

namespace
{
    constexpr int BLOCK = 256, WAVES = BLOCK / WAVE;
    constexpr int COLS = 4;                                  // columns per lane: one 16-byte access per stream
    constexpr int TX = 128, TY = 16;                         // nodes per tile
    constexpr int ROW_LANES = TX / COLS, ROWS = WAVE / ROW_LANES; // lanes per row; rows per wavefront pass
    constexpr int PASSES = TY / (WAVES * ROWS);
    static_assert(ROW_LANES * ROWS == WAVE && PASSES * WAVES * ROWS == TY, "a wavefront pass covers whole rows; the passes cover the tile");

    using V4 = float __attribute__((ext_vector_type(4)));
    using Lattice32 = LatticeT<float>;

    using StageArgs32 = StageArgsT<float>;

    // PSLOT > 0: input PSLOT of the stage is the stencil input itself
    template <typename Stage, int PSLOT, bool FORCED, bool NT, int NBT>
    __global__ void __launch_bounds__(BLOCK) weights32_kernel(Lattice32 L, StageArgs32 a, const float *__restrict__ weight)
    {
        constexpr int NIN = Stage::NIN + (FORCED ? 2 : 0), NOUT = Stage::NOUT;
        static_assert(NIN <= MAX_IN && NOUT <= MAX_OUT, "StageArgs32 holds every stage");
        constexpr int HM = (NBT ? NBT : NB_MAX) - 1, HP = (HM + COLS - 1) & ~(COLS - 1); // halo; the tile's first column sits at LDS column HP
        constexpr int LW = TX + 2 * HP, LG = LW / COLS;
        __shared__ __attribute__((aligned(16))) float tile[(TY + 2 * HM) * LW];
        __shared__ __attribute__((aligned(16))) float sT[(NB_MAX + 1) * 2 * NB_MAX];
        __shared__ float sWt[NB_MAX + 1];
        constexpr int HMIN = NBT ? NBT - 1 : 1, FX = (TX - 1) / HMIN + 2, FY = (TY - 1) / HMIN + 2; // cells that contain a node of the tile
        __shared__ float sF[FY * FX];
        static_assert(sizeof(tile) + sizeof(sT) + sizeof(sWt) + sizeof(sF) <= 64 * 1024, "static LDS of a workgroup");

        const int nb = NBT ? NBT : L.nb, H = nb - 1, WP = 2 * nb;
        const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;

        // this workgroup's tile: XCD x gets the x-th contiguous run of tiles
        const int ntx = (L.stride + TX - 1) / TX, n_tiles = gridDim.x;
        const int xcd = blockIdx.x % N_XCD, slot = blockIdx.x / N_XCD;
        const int t = xcd * (n_tiles / N_XCD) + min(xcd, n_tiles % N_XCD) + slot;
        const int tx0 = (t % ntx) * TX, ty0 = (t / ntx) * TY;

        // the cells around the tile's nodes: columns a0 .. , rows b0 .. ; a cell beyond the tile's last node or the grid has weight zero
        const int ncx = (L.Lx - 1) / H, ncy = (L.Ly - 1) / H;
        const int a0 = (tx0 + H - 1) / H - 1, b0 = (ty0 + H - 1) / H - 1;
        int any = 0;
        for (int i = tid; i < FY * FX; i += BLOCK)
        {
            const int bl = i / FX, al = i - bl * FX;
            const int ca = a0 + al, cb = b0 + bl;
            float f = 0.0f;
            if (ca >= 0 && ca < ncx && ca * H < tx0 + TX && cb >= 0 && cb < ncy && cb * H < ty0 + TY)
                f = weight[cb * ncx + ca];
            sF[i] = f;
            any |= f != 0.0f;
        }
        if (!__syncthreads_or(any))
            return;

        for (int i = tid; i < (nb + 1) * WP; i += BLOCK)
            sT[i] = L.T[i];
        if (tid <= nb)
            sWt[tid] = L.Wt[tid];
        const float *__restrict__ pin = a.in[0];
        for (int g = tid; g < (TY + 2 * H) * LG; g += BLOCK)
        {
            // tx0, HP and stride are multiples of four: a piece lies in its row or outside it
            const int jl = g / LG, il = COLS * (g - jl * LG);
            const int I = tx0 - HP + il, J = ty0 - H + jl;
            V4 piece = {0.0f, 0.0f, 0.0f, 0.0f};
            if (I >= 0 && I < L.stride && J >= 0 && J < L.Ly)
            {
                piece = *reinterpret_cast<const V4 *>(pin + J * L.stride + I);
#pragma unroll
                for (int c = 0; c < COLS; ++c)
                    piece[c] = I + c < L.Lx ? piece[c] : 0.0f;
            }
            *reinterpret_cast<V4 *>(tile + jl * LW + il) = piece;
        }
        __syncthreads();

        // what a lane's four columns need in every row
        const int lx = lane & (ROW_LANES - 1), half = lane / ROW_LANES;
        const int I0 = tx0 + COLS * lx;
        int rN[COLS], rR[COLS], loN[COLS], hiR[COLS], fL[COLS], fR[COLS], mL[COLS], mR[COLS];
        float wR[COLS];
        const float wL = sWt[H + 1];
#pragma unroll
        for (int c = 0; c < COLS; ++c)
        {
            const bool valid = I0 + c < L.Lx;
            const int I = valid ? I0 + c : tx0, kx = I % H;
            // d < 0 goes to one running sum: sL's row at an element boundary, the one sum's row kx inside an element
            rN[c] = kx == 0 ? H + 1 : kx;
            rR[c] = kx == 0 ? H : kx;
            loN[c] = valid ? (kx == 0 ? -H : -kx) : 0;
            hiR[c] = valid ? H - kx : 0;
            wR[c] = sWt[rR[c]];
            fR[c] = I / H - a0;
            fL[c] = kx == 0 ? fR[c] - 1 : fR[c];
            mR[c] = valid ? 1 : 0; // (a padding column has no cell)
            mL[c] = valid && kx == 0 ? 1 : 0;
        }
        const int ctr = HP + COLS * lx; // LDS column of I0

        V4 x[PASSES][NIN];
#pragma unroll
        for (int u = 0; u < PASSES; ++u)
        {
            // clamped, not guarded (blas1.hip, map_kernel)
            const int J = min(ty0 + ROWS * (wv + WAVES * u) + half, L.Ly - 1), I = min(I0, L.stride - COLS);
            const int i = (J * L.stride + I) / COLS;
#pragma unroll
            for (int s = 1; s < NIN; ++s)
                if (s != PSLOT)
                    x[u][s] = stream_load<NT>(reinterpret_cast<const V4 *>(a.in[s]) + i);
        }
#pragma unroll
        for (int u = 0; u < PASSES; ++u)
        {
            const int jt = ROWS * (wv + WAVES * u) + half, J = ty0 + jt;
            if (J < L.Ly && I0 < L.stride)
            {
                const int ky = J % H, rA = ky == 0 ? H : ky;
                const int rM = ky == 0 ? H + 1 : ky, loM = ky == 0 ? -H : -ky, hiA = H - ky;
                const float wB = sWt[H + 1], wA = sWt[rA];
                const int gA = (J / H - b0) * FX, gB = ky == 0 ? gA - FX : gA, mB = ky == 0 ? 1 : 0;
                const float *row = tile + (jt + H) * LW + ctr;
                // the offsets below zero run into one sum (sN along x, sM along y); at d = 0 an element boundary closes it as sL (sB)
                // and opens sR (sA) from zero, an element-interior node carries it on: the sums of wave_weights.hip, term by term
                float sN[COLS] = {0.0f, 0.0f, 0.0f, 0.0f}, sM[COLS] = {0.0f, 0.0f, 0.0f, 0.0f};
                float sL[COLS], sR[COLS], sB[COLS], sA[COLS];
                const float cL0 = sT[(H + 1) * WP + H], cA0 = sT[rA * WP + H];
                if constexpr (NBT != 0)
                {
                    float win[COLS + 2 * HP]; // columns I0 - HP .. I0 + COLS + HP - 1
#pragma unroll
                    for (int k = 0; k < COLS + 2 * HP; k += COLS)
                    {
                        const V4 piece = *reinterpret_cast<const V4 *>(row - HP + k);
#pragma unroll
                        for (int c = 0; c < COLS; ++c)
                            win[k + c] = piece[c];
                    }
#pragma unroll
                    for (int c = 0; c < COLS; ++c)
                    {
#pragma unroll
                        for (int d = -HM; d < 0; ++d)
                            if (d >= loN[c])
                                sN[c] = fmadd(sT[rN[c] * WP + d + H], win[HP + c + d], sN[c]);
                        const float p0 = win[HP + c];
                        sL[c] = mL[c] ? fmadd(cL0, p0, sN[c]) : 0.0f;
                        sR[c] = fmadd(sT[rR[c] * WP + H], p0, mL[c] ? 0.0f : sN[c]);
#pragma unroll
                        for (int d = 1; d <= HM; ++d)
                            if (d <= hiR[c])
                                sR[c] = fmadd(sT[rR[c] * WP + d + H], win[HP + c + d], sR[c]);
                        if constexpr (PSLOT > 0)
                            x[u][PSLOT][c] = p0;
                    }
#pragma unroll
                    for (int d = -HM; d <= HM; ++d)
                    {
                        const V4 piece = *reinterpret_cast<const V4 *>(row + d * LW); // (a halo row of the tile when out of range)
                        if (d < 0)
                        {
                            const float coef = sT[rM * WP + d + H];
                            if (d >= loM)
                            {
#pragma unroll
                                for (int c = 0; c < COLS; ++c)
                                    sM[c] = fmadd(coef, piece[c], sM[c]);
                            }
                        }
                        else if (d == 0)
                        {
#pragma unroll
                            for (int c = 0; c < COLS; ++c)
                            {
                                sB[c] = mB ? fmadd(cL0, piece[c], sM[c]) : 0.0f;
                                sA[c] = fmadd(cA0, piece[c], mB ? 0.0f : sM[c]);
                            }
                        }
                        else
                        {
                            const float coef = sT[rA * WP + d + H];
                            if (d <= hiA)
                            {
#pragma unroll
                                for (int c = 0; c < COLS; ++c)
                                    sA[c] = fmadd(coef, piece[c], sA[c]);
                            }
                        }
                    }
                }
                else
                {
#pragma unroll
                    for (int c = 0; c < COLS; ++c)
                    {
                        for (int d = loN[c]; d < 0; ++d)
                            sN[c] = fmadd(sT[rN[c] * WP + d + H], row[c + d], sN[c]);
                        const float p0 = row[c];
                        sL[c] = mL[c] ? fmadd(cL0, p0, sN[c]) : 0.0f;
                        sR[c] = fmadd(sT[rR[c] * WP + H], p0, mL[c] ? 0.0f : sN[c]);
                        for (int d = 1; d <= hiR[c]; ++d)
                            sR[c] = fmadd(sT[rR[c] * WP + d + H], row[c + d], sR[c]);
                        if constexpr (PSLOT > 0)
                            x[u][PSLOT][c] = p0;
                    }
                    for (int d = loM; d < 0; ++d)
                    {
                        const V4 piece = *reinterpret_cast<const V4 *>(row + d * LW);
                        const float coef = sT[rM * WP + d + H];
#pragma unroll
                        for (int c = 0; c < COLS; ++c)
                            sM[c] = fmadd(coef, piece[c], sM[c]);
                    }
                    {
                        const V4 piece = *reinterpret_cast<const V4 *>(row);
#pragma unroll
                        for (int c = 0; c < COLS; ++c)
                        {
                            sB[c] = mB ? fmadd(cL0, piece[c], sM[c]) : 0.0f;
                            sA[c] = fmadd(cA0, piece[c], mB ? 0.0f : sM[c]);
                        }
                    }
                    for (int d = 1; d <= hiA; ++d)
                    {
                        const V4 piece = *reinterpret_cast<const V4 *>(row + d * LW);
                        const float coef = sT[rA * WP + d + H];
#pragma unroll
                        for (int c = 0; c < COLS; ++c)
                            sA[c] = fmadd(coef, piece[c], sA[c]);
                    }
                }
                V4 y[NOUT];
#pragma unroll
                for (int c = 0; c < COLS; ++c)
                {
                    // the staged weight where the masks admit the cell (every index lies in the staged window)
                    const float fRA = mR[c] ? sF[gA + fR[c]] : 0.0f, fLA = mL[c] ? sF[gA + fL[c]] : 0.0f;
                    const float fRB = (mR[c] & mB) ? sF[gB + fR[c]] : 0.0f, fLB = (mL[c] & mB) ? sF[gB + fL[c]] : 0.0f;
                    const float aB = fmadd(fRB, sR[c], fLB * sL[c]), aA = fmadd(fRA, sR[c], fLA * sL[c]);
                    const float tx = fmadd(wA, aA, wB * aB);
                    const float bL = fmadd(fLA, sA[c], fLB * sB[c]), bR = fmadd(fRA, sA[c], fRB * sB[c]);
                    const float ty = fmadd(wR[c], bR, wL * bL);
                    const float kp = fmadd(L.cx, tx, L.cy * ty);
                    float xe[NIN], ye[NOUT];
                    xe[0] = (fRA != 0.0f || fLA != 0.0f || fRB != 0.0f || fLB != 0.0f) ? kp : 0.0f;
#pragma unroll
                    for (int s = 1; s < NIN; ++s)
                        xe[s] = x[u][s][c];
                    Stage::template apply<FORCED>(xe, ye, a.coef);
#pragma unroll
                    for (int s = 0; s < NOUT; ++s)
                        y[s][c] = ye[s];
                }
                const int i = (J * L.stride + I0) / COLS;
#pragma unroll
                for (int s = 0; s < NOUT; ++s)
                    stream_store<NT>(reinterpret_cast<V4 *>(a.out[s]) + i, y[s]);
            }
        }
    }

    // the family's launcher (wave_sweep_launch.hpp): one sweep on the entry points' leading arguments
    struct launch_weights32
    {
        const cuddh_wave_lattice *D;
        const float *weight;
        void *stream;

        template <typename Stage, int PSLOT>
        int sweep(const float *const (&in)[Stage::NIN], const float *F, const float *G, float *const (&out)[Stage::NOUT],
                  const double (&coef)[MAX_COEF]) const
        {
            Lattice32 L;
            StageArgs32 a;
            if (!describe(D, COLS, L) || !weight || !stage_args<Stage>(in, F, G, out, coef, a))
                return invalid_value;
            const int grid = ((L.stride + TX - 1) / TX) * ((L.Ly + TY - 1) / TY);
            dispatch_sweep(L.nb, NBasis<4, 5>{}, F != nullptr, static_cast<long long>(L.stride) * L.Ly * sizeof(float),
                           [&](auto forced_c, auto nt_c, auto nbt)
                           { hipLaunchKernelGGL((weights32_kernel<Stage, PSLOT, decltype(forced_c)::value, decltype(nt_c)::value, decltype(nbt)::value>),
                                                dim3(grid), dim3(BLOCK), 0, as_stream(stream), L, a, weight); });
            return launch_status();
        }
    };
} // namespace

extern "C"
{
    int cuddh_hip_wave_weights32_rk2_a(const cuddh_wave_lattice *lattice, const float *weight, double half_dt, double c, double s, const float *p, const float *q,
                               const float *invm, const float *Hi, const float *F, const float *G, float *qh, float *ph, void *stream)
    {
        return rk2_a(launch_weights32{lattice, weight, stream}, half_dt, c, s, p, q, invm, Hi, F, G, qh, ph);
    }

    int cuddh_hip_wave_weights32_rk2_b(const cuddh_wave_lattice *lattice, const float *weight, double dt, double c, double s, double filt, const float *ph, const float *qh,
                               const float *invm, const float *Hi, const float *F, const float *G, float *p, float *q, float *u, float *v,
                               void *stream)
    {
        return rk2_b(launch_weights32{lattice, weight, stream}, dt, c, s, filt, ph, qh, invm, Hi, F, G, p, q, u, v);
    }

    int cuddh_hip_wave_weights32_rk4_1(const cuddh_wave_lattice *lattice, const float *weight, double half_dt, double c, double s, const float *p, const float *q,
                               const float *invm, const float *Hi, const float *F, const float *G, float *ps, float *qs, float *aq, float *ap,
                               void *stream)
    {
        return rk4_1(launch_weights32{lattice, weight, stream}, half_dt, c, s, p, q, invm, Hi, F, G, ps, qs, aq, ap);
    }

    int cuddh_hip_wave_weights32_rk4_2(const cuddh_wave_lattice *lattice, const float *weight, double half_dt, double c, double s, const float *ps_in, const float *p,
                               const float *q, const float *invm, const float *Hi, const float *F, const float *G, float *ps_out, float *qs,
                               float *aq, float *ap, void *stream)
    {
        return rk4_2(launch_weights32{lattice, weight, stream}, half_dt, c, s, ps_in, p, q, invm, Hi, F, G, ps_out, qs, aq, ap);
    }

    int cuddh_hip_wave_weights32_rk4_3(const cuddh_wave_lattice *lattice, const float *weight, double dt, double c, double s, const float *ps_in, const float *p,
                               const float *q, const float *invm, const float *Hi, const float *F, const float *G, float *ps_out, float *qs,
                               float *aq, float *ap, void *stream)
    {
        return rk4_3(launch_weights32{lattice, weight, stream}, dt, c, s, ps_in, p, q, invm, Hi, F, G, ps_out, qs, aq, ap);
    }

    int cuddh_hip_wave_weights32_rk4_4(const cuddh_wave_lattice *lattice, const float *weight, double sixth_dt, double c, double s, double filt, const float *ps,
                               const float *qs, const float *aq, const float *ap, const float *invm, const float *Hi, const float *F,
                               const float *G, float *p, float *q, float *u, float *v, void *stream)
    {
        return rk4_4(launch_weights32{lattice, weight, stream}, sixth_dt, c, s, filt, ps, qs, aq, ap, invm, Hi, F, G, p, q, u, v);
    }
}
