// Lattice sweeps with a per-cell stiffness coefficient (csrc/src/waveholtz.cpp): the lattice of wave_lattice.hip, each
// of its nx x ny cells with a real weight beta (`weight`, nx ny doubles on the device, cell (a, b) at a + nx b).  The collocated
// stiffness of  -div(beta grad .), beta constant on each element, is the sum over the cells of beta_e times the element's Kronecker
// sum, regrouped per lattice node.  A cell of weight zero is a missing cell of wave_cells.hip.
//
// The stencil.  H = n_basis - 1, kx = I mod H, ky = J mod H, A the 1-D element matrix (row-major), w the weights, cx = hy / hx,
// cy = hx / hy.  Along x a node has two sums, each from zero, d ascending, by fma:
//   kx = 0:      sL = sum_{d = -H..0} A[H][H + d] p(I + d, J)   (the cell column to the left,  I / H - 1),   wL = w[H]
//                sR = sum_{d = 0..H}  A[0][d]     p(I + d, J)   (the cell column to the right, I / H),       wR = w[0]
//   0 < kx < H:  sR = sum_{d = -kx..H - kx} A[kx][kx + d] p(I + d, J)   (the one column I / H),  wR = w[kx];   sL = 0, no left column
// and along y likewise sB, wB (the cell row below, J / H - 1) and sA, wA (the row above or the one row, J / H).  p outside the
// lattice counts as zero and a cell column or row outside the grid as weight zero, so at I = 0 and I = Lx - 1 only the side that
// exists contributes.  With f_XY the weight of the cell in column X and row Y, and 0.0 where there is no such cell:
//   aB = fma(f_RB, sR, f_LB sL),   aA = fma(f_RA, sR, f_LA sL),   tx = fma(wA, aA, wB aB)
//   bL = fma(f_LA, sA, f_LB sB),   bR = fma(f_RA, sA, f_RB sB),   ty = fma(wR, bR, wL bL)
//   (K p)(I, J) = fma(cx, tx, cy ty)
// and (K p)(I, J) = +0 where all four weights are zero (a void node; its invm is zero, so the stages keep its state zero, as they do
// for padding).  The order depends on (I, J) only: results are bitwise reproducible, and with weights in {0, 1} they are the bits of
// wave_cells.hip, whose terms these are in its order.  The kernels do not inspect the weights: finiteness and sign are the host's.
//
// Layout, decomposition, streams, workgroup renumbering and the n_basis instantiations are wave_lattice.hip's.  A tile first stages
// the weights of the cells that contain one of its nodes (at most (TX - 1) / H + 2 by (TY - 1) / H + 2) in LDS; when all of them
// are zero the workgroup returns: it loads and stores no vector, so the outputs keep what they held there.
// The tables are wave::describe's: row H of T is A[0][.], row H + 1 is A[H][.], row k is A[k][.]; Wt[H] = w[0], Wt[H + 1] = w[H].
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
    constexpr int TX = 128, TY = 16; // nodes per tile; TX = 2 columns per lane
    constexpr int ROWS_PER_WAVE = TY / WAVES, UNROLL = 2;
    static_assert(TX == 2 * WAVE && ROWS_PER_WAVE % UNROLL == 0, "a lane owns two columns; rows go in pairs");

    using Lattice = LatticeT<double>;

    // PSLOT > 0: input PSLOT of the stage is the stencil input itself
    template <typename Stage, int PSLOT, bool FORCED, bool NT, int NBT>
    __global__ void __launch_bounds__(BLOCK) weights_kernel(Lattice L, StageArgs a, const double *__restrict__ weight)
    {
        constexpr int NIN = Stage::NIN + (FORCED ? 2 : 0), NOUT = Stage::NOUT;
        static_assert(NIN <= MAX_IN && NOUT <= MAX_OUT, "StageArgs holds every stage");
        constexpr int HM = (NBT ? NBT : NB_MAX) - 1, HP = (HM + 1) & ~1; // halo; the tile's first column sits at LDS column HP (even)
        constexpr int LW = TX + 2 * HP;
        constexpr int HMIN = NBT ? NBT - 1 : 1, FX = (TX - 1) / HMIN + 2, FY = (TY - 1) / HMIN + 2; // cells that contain a node of the tile
        __shared__ __attribute__((aligned(16))) double tile[(TY + 2 * HM) * LW];
        __shared__ __attribute__((aligned(16))) double sT[(NB_MAX + 1) * 2 * NB_MAX];
        __shared__ double sWt[NB_MAX + 1];
        __shared__ double sF[FY * FX];
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
            double f = 0.0;
            if (ca >= 0 && ca < ncx && ca * H < tx0 + TX && cb >= 0 && cb < ncy && cb * H < ty0 + TY)
                f = weight[cb * ncx + ca];
            sF[i] = f;
            any |= f != 0.0;
        }
        if (!__syncthreads_or(any))
            return;

        for (int i = tid; i < (nb + 1) * WP; i += BLOCK)
            sT[i] = L.T[i];
        if (tid <= nb)
            sWt[tid] = L.Wt[tid];
        const double *__restrict__ pin = a.in[0];
        for (int i = tid; i < (TY + 2 * H) * LW; i += BLOCK)
        {
            const int jl = i / LW, il = i - jl * LW;
            const int I = tx0 - HP + il, J = ty0 - H + jl;
            tile[i] = (I >= 0 && I < L.Lx && J >= 0 && J < L.Ly) ? pin[J * L.stride + I] : 0.0;
        }
        __syncthreads();

        // what a lane's two columns need in every row: the rows of T and the offset ranges of sL and sR, the weights, the cell columns
        const int I0 = tx0 + 2 * lane;
        int rN[2], rR[2], loN[2], hiR[2], fL[2], fR[2], mL[2], mR[2];
        double wL[2], wR[2];
#pragma unroll
        for (int c = 0; c < 2; ++c)
        {
            const bool valid = I0 + c < L.Lx;
            const int I = valid ? I0 + c : tx0, kx = I % H;
            // d < 0 goes to one running sum: sL's row at an element boundary, the one sum's row kx inside an element
            rN[c] = kx == 0 ? H + 1 : kx;
            rR[c] = kx == 0 ? H : kx;
            loN[c] = valid ? (kx == 0 ? -H : -kx) : 0;
            hiR[c] = valid ? H - kx : 0;
            wL[c] = sWt[H + 1];
            wR[c] = sWt[rR[c]];
            fR[c] = I / H - a0;
            fL[c] = kx == 0 ? fR[c] - 1 : fR[c];
            mR[c] = valid ? 1 : 0; // (a padding column has no cell)
            mL[c] = valid && kx == 0 ? 1 : 0;
        }
        const int ctr = HP + 2 * lane; // LDS column of I0

        for (int m0 = 0; m0 < ROWS_PER_WAVE; m0 += UNROLL)
        {
            V2 x[UNROLL][NIN];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
            {
                // clamped, not guarded (blas1.hip, map_kernel)
                const int J = min(ty0 + wv + WAVES * (m0 + u), L.Ly - 1), I = min(I0, L.stride - 2);
                const int i = (J * L.stride + I) / 2;
#pragma unroll
                for (int s = 1; s < NIN; ++s)
                    if (s != PSLOT)
                        x[u][s] = stream_load<NT>(reinterpret_cast<const V2 *>(a.in[s]) + i);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
            {
                const int jt = wv + WAVES * (m0 + u), J = ty0 + jt;
                if (J < L.Ly && I0 < L.stride)
                {
                    const int ky = J % H, rA = ky == 0 ? H : ky;
                    const int rM = ky == 0 ? H + 1 : ky, loM = ky == 0 ? -H : -ky, hiA = H - ky;
                    const double wB = sWt[H + 1], wA = sWt[rA];
                    const int gA = (J / H - b0) * FX, gB = ky == 0 ? gA - FX : gA;
                    const int mB = ky == 0 ? 1 : 0;
                    const double *row = tile + (jt + H) * LW + ctr;
#pragma unroll
                    for (int c = 0; c < 2; ++c)
                    {
                        // the offsets below zero run into one sum; at d = 0 an element boundary closes it as sL (sB) and opens sR (sA)
                        // from zero, an element-interior node carries it on: the sums of the head of this file, term by term
                        double sN = 0.0, sM = 0.0;
#pragma unroll
                        for (int d = -HM; d < 0; ++d)
                            if (d >= loN[c])
                                sN = fmadd(sT[rN[c] * WP + d + H], row[c + d], sN);
#pragma unroll
                        for (int d = -HM; d < 0; ++d)
                            if (d >= loM)
                                sM = fmadd(sT[rM * WP + d + H], row[c + d * LW], sM);
                        const double p0 = row[c];
                        const double sL = mL[c] ? fmadd(sT[(H + 1) * WP + H], p0, sN) : 0.0;
                        const double sB = mB ? fmadd(sT[(H + 1) * WP + H], p0, sM) : 0.0;
                        double sR = fmadd(sT[rR[c] * WP + H], p0, mL[c] ? 0.0 : sN);
                        double sA = fmadd(sT[rA * WP + H], p0, mB ? 0.0 : sM);
#pragma unroll
                        for (int d = 1; d <= HM; ++d)
                            if (d <= hiR[c])
                                sR = fmadd(sT[rR[c] * WP + d + H], row[c + d], sR);
#pragma unroll
                        for (int d = 1; d <= HM; ++d)
                            if (d <= hiA)
                                sA = fmadd(sT[rA * WP + d + H], row[c + d * LW], sA);
                        // the staged weight where the masks admit the cell (every index lies in the staged window)
                        const double fRA = mR[c] ? sF[gA + fR[c]] : 0.0, fLA = mL[c] ? sF[gA + fL[c]] : 0.0;
                        const double fRB = (mR[c] & mB) ? sF[gB + fR[c]] : 0.0, fLB = (mL[c] & mB) ? sF[gB + fL[c]] : 0.0;
                        const double aB = fmadd(fRB, sR, fLB * sL), aA = fmadd(fRA, sR, fLA * sL);
                        const double tx = fmadd(wA, aA, wB * aB);
                        const double bL = fmadd(fLA, sA, fLB * sB), bR = fmadd(fRA, sA, fRB * sB);
                        const double ty = fmadd(wR[c], bR, wL[c] * bL);
                        const double kp = fmadd(L.cx, tx, L.cy * ty);
                        x[u][0][c] = (fRA != 0.0 || fLA != 0.0 || fRB != 0.0 || fLB != 0.0) ? kp : 0.0;
                        if constexpr (PSLOT > 0)
                            x[u][PSLOT][c] = row[c];
                    }
                    V2 y[NOUT];
#pragma unroll
                    for (int c = 0; c < 2; ++c)
                    {
                        double xe[NIN], ye[NOUT];
#pragma unroll
                        for (int s = 0; s < NIN; ++s)
                            xe[s] = x[u][s][c];
                        Stage::template apply<FORCED>(xe, ye, a.coef);
#pragma unroll
                        for (int s = 0; s < NOUT; ++s)
                            y[s][c] = ye[s];
                    }
                    const int i = (J * L.stride + I0) / 2;
#pragma unroll
                    for (int s = 0; s < NOUT; ++s)
                        stream_store<NT>(reinterpret_cast<V2 *>(a.out[s]) + i, y[s]);
                }
            }
        }
    }

    // the family's launcher (wave_sweep_launch.hpp): one sweep on the entry points' leading arguments
    struct launch_weights
    {
        const cuddh_wave_lattice *D;
        const double *weight;
        void *stream;

        template <typename Stage, int PSLOT>
        int sweep(const double *const (&in)[Stage::NIN], const double *F, const double *G, double *const (&out)[Stage::NOUT],
                  const double (&coef)[MAX_COEF]) const
        {
            Lattice L;
            StageArgs a;
            if (!describe(D, 2, L) || !weight || !stage_args<Stage>(in, F, G, out, coef, a))
                return invalid_value;
            const int grid = ((L.stride + TX - 1) / TX) * ((L.Ly + TY - 1) / TY);
            dispatch_sweep(L.nb, NBasis<4, 5>{}, F != nullptr, static_cast<long long>(L.stride) * L.Ly * sizeof(double),
                           [&](auto forced_c, auto nt_c, auto nbt)
                           { hipLaunchKernelGGL((weights_kernel<Stage, PSLOT, decltype(forced_c)::value, decltype(nt_c)::value, decltype(nbt)::value>),
                                                dim3(grid), dim3(BLOCK), 0, as_stream(stream), L, a, weight); });
            return launch_status();
        }
    };
} // namespace

extern "C"
{
    int cuddh_hip_wave_weights_rk2_a_f64(const cuddh_wave_lattice *lattice, const double *weight, double half_dt, double c, double s,
                                         const double *p, const double *q, const double *invm, const double *Hi, const double *F, const double *G,
                                         double *qh, double *ph, void *stream)
    {
        return rk2_a(launch_weights{lattice, weight, stream}, half_dt, c, s, p, q, invm, Hi, F, G, qh, ph);
    }

    int cuddh_hip_wave_weights_rk2_b_f64(const cuddh_wave_lattice *lattice, const double *weight, double dt, double c, double s, double filt,
                                         const double *ph, const double *qh, const double *invm, const double *Hi, const double *F, const double *G,
                                         double *p, double *q, double *u, double *v, void *stream)
    {
        return rk2_b(launch_weights{lattice, weight, stream}, dt, c, s, filt, ph, qh, invm, Hi, F, G, p, q, u, v);
    }

    int cuddh_hip_wave_weights_rk4_1_f64(const cuddh_wave_lattice *lattice, const double *weight, double half_dt, double c, double s,
                                         const double *p, const double *q, const double *invm, const double *Hi, const double *F, const double *G,
                                         double *ps, double *qs, double *aq, double *ap, void *stream)
    {
        return rk4_1(launch_weights{lattice, weight, stream}, half_dt, c, s, p, q, invm, Hi, F, G, ps, qs, aq, ap);
    }

    int cuddh_hip_wave_weights_rk4_2_f64(const cuddh_wave_lattice *lattice, const double *weight, double half_dt, double c, double s,
                                         const double *ps_in, const double *p, const double *q, const double *invm, const double *Hi, const double *F,
                                         const double *G, double *ps_out, double *qs, double *aq, double *ap, void *stream)
    {
        return rk4_2(launch_weights{lattice, weight, stream}, half_dt, c, s, ps_in, p, q, invm, Hi, F, G, ps_out, qs, aq, ap);
    }

    int cuddh_hip_wave_weights_rk4_3_f64(const cuddh_wave_lattice *lattice, const double *weight, double dt, double c, double s,
                                         const double *ps_in, const double *p, const double *q, const double *invm, const double *Hi, const double *F,
                                         const double *G, double *ps_out, double *qs, double *aq, double *ap, void *stream)
    {
        return rk4_3(launch_weights{lattice, weight, stream}, dt, c, s, ps_in, p, q, invm, Hi, F, G, ps_out, qs, aq, ap);
    }

    int cuddh_hip_wave_weights_rk4_4_f64(const cuddh_wave_lattice *lattice, const double *weight, double sixth_dt, double c, double s, double filt,
                                         const double *ps, const double *qs, const double *aq, const double *ap, const double *invm, const double *Hi,
                                         const double *F, const double *G, double *p, double *q, double *u, double *v, void *stream)
    {
        return rk4_4(launch_weights{lattice, weight, stream}, sixth_dt, c, s, filt, ps, qs, aq, ap, invm, Hi, F, G, p, q, u, v);
    }
}
