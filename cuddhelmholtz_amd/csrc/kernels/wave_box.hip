// Box sweeps of the whole-domain WaveHoltz march in three dimensions (csrc/src/waveholtz_box.cpp): on a box of
// nx x ny x nz congruent brick elements the collocated (Gauss-Lobatto) stiffness is a Kronecker sum on the global lattice of
// Lx x Ly x Lz Gauss-Lobatto nodes,
//   K = cx Wz (x) Wy (x) Ax  +  cy Wz (x) Ay (x) Wx  +  cz Az (x) Wy (x) Wx,     node (I, J, K) at I + stride (J + Ly K),
//   cx = hy hz / (2 hx),  cy = hx hz / (2 hy),  cz = hx hy / (2 hz),
// A., W. the 1-D element matrix and weights of wave_lattice.hip assembled along a line of elements.  ONE launch does a whole
// Runge-Kutta sweep: the stencil, then the stage of wave_stages.hpp with x[0] computed instead of loaded.
//
// The stencil.  Row ids r, offset ranges and the tables T[r][d], Wt[r] are wave_lattice.hip's (wave_lattice_common.hpp), one line
// per direction.  With rx = r(I), ry = r(J), rz = r(K):
//   sx = sum_d T[rx][d] p(I + d, J, K),   sy = sum_d T[ry][d] p(I, J + d, K),   sz = sum_d T[rz][d] p(I, J, K + d),
//        each from zero, d ascending over the node's range, by fma;
//   ax = cx * (Wt[ry] * Wt[rz]),   ay = cy * (Wt[rx] * Wt[rz]),   az = cz * (Wt[rx] * Wt[ry]),   each product rounded, the inner first;
//   (K p)(I, J, K) = fma(ax, sx, fma(ay, sy, az * sz)).
// The order depends on nothing but (I, J, K): results are bitwise reproducible.  Offsets outside a node's range are not read.
//
// Layout.  Rows have `stride` >= Lx doubles, stride even; the columns from Lx on are padding that holds zero state, zero load and
// invm = 0 (the march keeps them zero).  The stencil never uses them: a padding column's sums are taken as zero.
//
// Decomposition.  A workgroup of four wavefronts owns a tile of TX x TY nodes of ONE z plane.  The plane's part of the stencil is
// wave_lattice.hip's: the tile and its halo of H rows and columns staged in LDS, a lane two neighbouring columns, rows in pairs.
// The z term reads its up to 2 H neighbours of the other planes straight from memory, one cached 16-byte load per plane and lane
// (the centre comes from the tile): nothing of another plane is shared between the lanes of a workgroup, so LDS would only copy
// it.  What makes those loads cheap is the numbering: workgroup ids are renumbered so that each XCD (ids are dealt round robin over
// eight) gets a contiguous run of tiles, and the tiles are numbered with z fastest, so that the workgroups resident on an XCD at
// one time are neighbouring planes of few x-y tiles and meet each other's planes in that XCD's L2.  A walk along z that keeps a
// layer of planes in LDS is not built.
// n_basis 4 is compile-time: its z loads are all issued before the first is used.  Every other n_basis in [2, 8] shares an
// instantiation whose x and y loops have run-time bounds over LDS and whose z loop has a run-time length (no register arrays,
// hence no scratch).
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
    constexpr int TX = 128, TY = 16, TZ = 1; // nodes per tile; TX = 2 columns per lane
    constexpr int ROWS_PER_WAVE = TY / WAVES, UNROLL = 2;
    static_assert(TX == 2 * WAVE && ROWS_PER_WAVE % UNROLL == 0, "a lane owns two columns; rows go in pairs");

    using Box = BoxT<double>; // (wave_lattice_common.hpp)

    template <int NBT>
    struct Lds
    {
        static constexpr int HM = (NBT ? NBT : NB_MAX) - 1, HP = (HM + 1) & ~1; // halo; the tile's first column sits at LDS column HP (even)
        static constexpr int LW = TX + 2 * HP, TILE = (TY + 2 * HM) * LW, TABLE = (NB_MAX + 1) * 2 * NB_MAX;
        static constexpr int BYTES = (TILE + TABLE + NB_MAX + 1) * static_cast<int>(sizeof(double));
    };
    static_assert(Lds<4>::BYTES <= 64 * 1024, "n_basis 4: at most 64 KB of LDS per workgroup");
    static_assert(Lds<0>::BYTES <= 64 * 1024, "run-time n_basis: at most 64 KB of LDS per workgroup");

    // PSLOT > 0: input PSLOT of the stage is the stencil input itself
    template <typename Stage, int PSLOT, bool FORCED, bool NT, int NBT>
    __global__ void __launch_bounds__(BLOCK) box_kernel(Box B, StageArgs a)
    {
        constexpr int NIN = Stage::NIN + (FORCED ? 2 : 0), NOUT = Stage::NOUT;
        static_assert(NIN <= MAX_IN && NOUT <= MAX_OUT, "StageArgs holds every stage");
        constexpr int HM = Lds<NBT>::HM, HP = Lds<NBT>::HP, LW = Lds<NBT>::LW;
        __shared__ __attribute__((aligned(16))) double tile[Lds<NBT>::TILE];
        __shared__ __attribute__((aligned(16))) double sT[Lds<NBT>::TABLE];
        __shared__ double sWt[NB_MAX + 1];

        const LatticeT<double> &L = B.L;
        const int nb = NBT ? NBT : L.nb, H = nb - 1, WP = 2 * nb;
        const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;

        // this workgroup's tile: XCD x gets the x-th contiguous run of tiles, z fastest
        const int ntx = (L.stride + TX - 1) / TX, n_tiles = gridDim.x;
        const int xcd = blockIdx.x % N_XCD, slot = blockIdx.x / N_XCD;
        const int t = xcd * (n_tiles / N_XCD) + min(xcd, n_tiles % N_XCD) + slot;
        const int Kz = t % B.Lz, txy = t / B.Lz;
        const int tx0 = (txy % ntx) * TX, ty0 = (txy / ntx) * TY;
        const int plane = L.stride * L.Ly; // (stride Ly Lz fits in an int)

        for (int i = tid; i < (nb + 1) * WP; i += BLOCK)
            sT[i] = L.T[i];
        if (tid <= nb)
            sWt[tid] = L.Wt[tid];
        const double *__restrict__ pin = a.in[0];
        const double *__restrict__ pk = pin + static_cast<size_t>(Kz) * plane;
        for (int i = tid; i < (TY + 2 * H) * LW; i += BLOCK)
        {
            const int jl = i / LW, il = i - jl * LW;
            const int I = tx0 - HP + il, J = ty0 - H + jl;
            tile[i] = (I >= 0 && I < L.Lx && J >= 0 && J < L.Ly) ? pk[J * L.stride + I] : 0.0;
        }
        __syncthreads();

        // what a lane's two columns need in every row
        const int I0 = tx0 + 2 * lane;
        int rx[2], lox[2], hix[2];
        double wx[2];
        bool valid[2];
#pragma unroll
        for (int c = 0; c < 2; ++c)
        {
            valid[c] = I0 + c < L.Lx;
            rx[c] = valid[c] ? row_id(I0 + c, L.Lx, nb) : 0;
            lox[c] = valid[c] ? first_offset(rx[c], nb) : 1;
            hix[c] = valid[c] ? last_offset(rx[c], nb) : 0;
            wx[c] = valid[c] ? sWt[rx[c]] : 0.0;
        }
        const int ctr = HP + 2 * lane; // LDS column of I0
        // the plane's row of the z line: the same for the whole workgroup
        const int rz = row_id(Kz, B.Lz, nb), loz = first_offset(rz, nb), hiz = last_offset(rz, nb);
        const double wz = sWt[rz];
        const double ay[2] = {L.cy * (wx[0] * wz), L.cy * (wx[1] * wz)};

        for (int m0 = 0; m0 < ROWS_PER_WAVE; m0 += UNROLL)
        {
            V2 x[UNROLL][NIN];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
            {
                // clamped, not guarded (blas1.hip, map_kernel)
                const int J = min(ty0 + wv + WAVES * (m0 + u), L.Ly - 1), I = min(I0, L.stride - 2);
                const size_t i = (static_cast<size_t>(Kz) * plane + J * L.stride + I) / 2;
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
                    const int ry = row_id(J, L.Ly, nb), loy = first_offset(ry, nb), hiy = last_offset(ry, nb);
                    const double wy = sWt[ry];
                    const double ax = L.cx * (wy * wz);
                    const double *row = tile + (jt + H) * LW + ctr;
                    // the z line of this lane's two columns: plane Kz + d at zl[d * plane / 2]
                    const V2 *zl = reinterpret_cast<const V2 *>(pk + J * L.stride + I0);
                    V2 sz = {0.0, 0.0};
                    if constexpr (NBT != 0)
                    {
                        V2 zv[2 * HM + 1];
#pragma unroll
                        for (int d = -HM; d <= HM; ++d)
                            if (d != 0)
                                zv[d + HM] = zl[static_cast<ptrdiff_t>(min(max(Kz + d, 0), B.Lz - 1) - Kz) * (plane / 2)]; // clamped; used in range only
#pragma unroll
                        for (int d = -HM; d <= HM; ++d)
                            if (d >= loz && d <= hiz)
                            {
                                const double tz = sT[rz * WP + d + H];
                                const V2 pz = d == 0 ? V2{row[0], row[1]} : zv[d + HM];
                                sz[0] = fmadd(tz, pz[0], sz[0]);
                                sz[1] = fmadd(tz, pz[1], sz[1]);
                            }
                    }
                    else
                    {
                        for (int d = loz; d <= hiz; ++d)
                        {
                            const double tz = sT[rz * WP + d + H];
                            const V2 pz = zl[static_cast<ptrdiff_t>(d) * (plane / 2)];
                            sz[0] = fmadd(tz, pz[0], sz[0]);
                            sz[1] = fmadd(tz, pz[1], sz[1]);
                        }
                    }
#pragma unroll
                    for (int c = 0; c < 2; ++c)
                    {
                        double sx = 0.0, sy = 0.0;
#pragma unroll
                        for (int d = -HM; d <= HM; ++d)
                            if (d >= lox[c] && d <= hix[c])
                                sx = fmadd(sT[rx[c] * WP + d + H], row[c + d], sx);
#pragma unroll
                        for (int d = -HM; d <= HM; ++d)
                            if (d >= loy && d <= hiy)
                                sy = fmadd(sT[ry * WP + d + H], row[c + d * LW], sy);
                        const double az = B.cz * (wx[c] * wy);
                        x[u][0][c] = fmadd(ax, sx, fmadd(ay[c], sy, az * (valid[c] ? sz[c] : 0.0)));
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
                    const size_t i = (static_cast<size_t>(Kz) * plane + J * L.stride + I0) / 2;
#pragma unroll
                    for (int s = 0; s < NOUT; ++s)
                        stream_store<NT>(reinterpret_cast<V2 *>(a.out[s]) + i, y[s]);
                }
            }
        }
    }

    // the family's launcher (wave_sweep_launch.hpp): one sweep on the entry points' leading arguments
    struct launch_box
    {
        const cuddh_wave_box *D;
        void *stream;

        template <typename Stage, int PSLOT>
        int sweep(const double *const (&in)[Stage::NIN], const double *F, const double *G, double *const (&out)[Stage::NOUT],
                  const double (&coef)[MAX_COEF]) const
        {
            Box B;
            StageArgs a;
            if (!describe_box(D, 2, B) || !stage_args<Stage>(in, F, G, out, coef, a))
                return invalid_value;
            const long long tiles = static_cast<long long>((B.L.stride + TX - 1) / TX) * ((B.L.Ly + TY - 1) / TY) * B.Lz;
            if (tiles > 0x7fffffffLL)
                return invalid_value;
            const int grid = static_cast<int>(tiles);
            dispatch_sweep(B.L.nb, NBasis<4>{}, F != nullptr, static_cast<long long>(B.L.stride) * B.L.Ly * B.Lz * sizeof(double),
                           [&](auto forced_c, auto nt_c, auto nbt)
                           { hipLaunchKernelGGL((box_kernel<Stage, PSLOT, decltype(forced_c)::value, decltype(nt_c)::value, decltype(nbt)::value>),
                                                dim3(grid), dim3(BLOCK), 0, as_stream(stream), B, a); });
            return launch_status();
        }
    };
} // namespace

extern "C"
{
    int cuddh_hip_wave_box_tile_x(void) { return TX; }
    int cuddh_hip_wave_box_tile_y(void) { return TY; }
    int cuddh_hip_wave_box_tile_z(void) { return TZ; }

    int cuddh_hip_wave_box_rk2_a_f64(const cuddh_wave_box *box, double half_dt, double c, double s, const double *p, const double *q,
                                     const double *invm, const double *Hi, const double *F, const double *G, double *qh, double *ph, void *stream)
    {
        return rk2_a(launch_box{box, stream}, half_dt, c, s, p, q, invm, Hi, F, G, qh, ph);
    }

    int cuddh_hip_wave_box_rk2_b_f64(const cuddh_wave_box *box, double dt, double c, double s, double filt, const double *ph, const double *qh,
                                     const double *invm, const double *Hi, const double *F, const double *G, double *p, double *q, double *u,
                                     double *v, void *stream)
    {
        return rk2_b(launch_box{box, stream}, dt, c, s, filt, ph, qh, invm, Hi, F, G, p, q, u, v);
    }

    int cuddh_hip_wave_box_rk4_1_f64(const cuddh_wave_box *box, double half_dt, double c, double s, const double *p, const double *q,
                                     const double *invm, const double *Hi, const double *F, const double *G, double *ps, double *qs, double *aq,
                                     double *ap, void *stream)
    {
        return rk4_1(launch_box{box, stream}, half_dt, c, s, p, q, invm, Hi, F, G, ps, qs, aq, ap);
    }

    int cuddh_hip_wave_box_rk4_2_f64(const cuddh_wave_box *box, double half_dt, double c, double s, const double *ps_in, const double *p,
                                     const double *q, const double *invm, const double *Hi, const double *F, const double *G, double *ps_out,
                                     double *qs, double *aq, double *ap, void *stream)
    {
        return rk4_2(launch_box{box, stream}, half_dt, c, s, ps_in, p, q, invm, Hi, F, G, ps_out, qs, aq, ap);
    }

    int cuddh_hip_wave_box_rk4_3_f64(const cuddh_wave_box *box, double dt, double c, double s, const double *ps_in, const double *p,
                                     const double *q, const double *invm, const double *Hi, const double *F, const double *G, double *ps_out,
                                     double *qs, double *aq, double *ap, void *stream)
    {
        return rk4_3(launch_box{box, stream}, dt, c, s, ps_in, p, q, invm, Hi, F, G, ps_out, qs, aq, ap);
    }

    int cuddh_hip_wave_box_rk4_4_f64(const cuddh_wave_box *box, double sixth_dt, double c, double s, double filt, const double *ps,
                                     const double *qs, const double *aq, const double *ap, const double *invm, const double *Hi, const double *F,
                                     const double *G, double *p, double *q, double *u, double *v, void *stream)
    {
        return rk4_4(launch_box{box, stream}, sixth_dt, c, s, filt, ps, qs, aq, ap, invm, Hi, F, G, p, q, u, v);
    }
}
