// The box lattice of the three-dimensional whole-domain WaveHoltz solver (cuddh/wave_box.hpp): description, lumped mass, lumped
// face mass and slot maps.  Plain host code.
#include "cuddh/wave_box.hpp"

#include <cmath>
#include <string>

#include "cuddh/basis.hpp"
#include "cuddh/error.hpp"
#include "cuddh/wave_lattice.hpp"

namespace cuddh
{
    namespace
    {
        void refuse(const std::string &what) { cuddh_error(("WaveHoltz error: box: " + what).c_str()); }

        /// the weights w assembled along a line of n elements that overlap in one node
        std::vector<double> line_weights(int n, int nb, const double *w)
        {
            const int H = nb - 1, L = n * H + 1;
            std::vector<double> W(L);
            const double joint = w[H] + w[0];
            for (int i = 0; i < L; ++i)
                W[i] = i == 0 ? w[0] : (i == L - 1 ? w[H] : (i % H == 0 ? joint : w[i % H]));
            return W;
        }
    } // namespace

    double check_wave_box(int nx, int ny, int nz, const double *box, int n_basis, const double *h_a, unsigned face_mask, int row_multiple)
    {
        const int counts[3] = {nx, ny, nz};
        const char *axis[3] = {"x", "y", "z"};
        for (int d = 0; d < 3; ++d)
            if (counts[d] < 1)
                refuse(std::string("the box needs at least one element in ") + axis[d] + ", not " + std::to_string(counts[d]) + ".");
        if (!box)
            refuse("no intervals were given (NULL).");
        for (int d = 0; d < 3; ++d)
            if (!std::isfinite(box[2 * d]) || !std::isfinite(box[2 * d + 1]) || !(box[2 * d] < box[2 * d + 1]))
                refuse(std::string("the interval in ") + axis[d] + " is empty, inverted or not finite: [" + std::to_string(box[2 * d]) + ", " +
                       std::to_string(box[2 * d + 1]) + "].");
        if (n_basis < 2 || n_basis > 8)
            refuse("the box kernels take n_basis in [2, 8], not " + std::to_string(n_basis) + ".");
        if (face_mask > WaveBox::all_faces)
            refuse("the face mask has six bits (x0, x1, y0, y1, z0, z1), not " + std::to_string(face_mask) + ".");
        if (row_multiple != 2 && row_multiple != 4)
            refuse("rows hold a multiple of 2 (fp64) or 4 (fp32) elements, not of " + std::to_string(row_multiple) + ".");
        const long long H = n_basis - 1, Lx = nx * H + 1, Ly = ny * H + 1, Lz = nz * H + 1, stride = (Lx + row_multiple - 1) / row_multiple * row_multiple;
        if (Lx > 0x7fffffffLL || Ly > 0x7fffffffLL || Lz > 0x7fffffffLL || stride * Ly > 0x7fffffffLL || stride * Ly * Lz > 0x7fffffffLL)
            refuse("the padded lattice of " + std::to_string(stride) + " x " + std::to_string(Ly) + " x " + std::to_string(Lz) +
                   " slots does not fit in an int.");
        double a_min = 1.0;
        if (h_a)
        {
            a_min = INFINITY;
            const long long n = Lx * Ly * Lz;
            for (long long g = 0; g < n; ++g)
            {
                if (!std::isfinite(h_a[g]) || !(h_a[g] > 0.0))
                    refuse("a = " + std::to_string(h_a[g]) + " at node " + std::to_string(g) + "; a must be finite and positive.");
                a_min = std::fmin(a_min, h_a[g]);
            }
        }
        return a_min;
    }

    WaveBox build_wave_box(int nx, int ny, int nz, const double *box, int n_basis, const double *h_a, unsigned face_mask, int row_multiple)
    {
        check_wave_box(nx, ny, nz, box, n_basis, h_a, face_mask, row_multiple);
        WaveBox B;
        const int nb = n_basis, H = nb - 1;
        B.Lx = nx * H + 1;
        B.Ly = ny * H + 1;
        B.Lz = nz * H + 1;
        B.hx = (box[1] - box[0]) / nx;
        B.hy = (box[3] - box[2]) / ny;
        B.hz = (box[5] - box[4]) / nz;
        const double hx = B.hx, hy = B.hy, hz = B.hz;
        B.desc.nx = nx;
        B.desc.ny = ny;
        B.desc.nz = nz;
        B.desc.n_basis = nb;
        B.desc.stride = (B.Lx + row_multiple - 1) / row_multiple * row_multiple;
        B.desc.cx = hy * hz / (2.0 * hx);
        B.desc.cy = hx * hz / (2.0 * hy);
        B.desc.cz = hx * hy / (2.0 * hz);
        wave_lattice_tables(Basis(nb), B.desc.A, B.desc.w);
        const std::vector<double> Wx = line_weights(nx, nb, B.desc.w), Wy = line_weights(ny, nb, B.desc.w), Wz = line_weights(nz, nb, B.desc.w);
        const int Lx = B.Lx, Ly = B.Ly, Lz = B.Lz, stride = B.desc.stride, n = B.nodes();
        B.m.resize(n);
        B.h.resize(n);
        B.invm.resize(n);
        B.Hi.resize(n);
        B.slot_of_dof.resize(n);
        B.dof_of_slot.assign(B.slots(), -1);
        const double cm = hx * hy * hz / 8.0, fx = hy * hz / 4.0, fy = hx * hz / 4.0, fz = hx * hy / 4.0;
        for (int K = 0; K < Lz; ++K)
            for (int J = 0; J < Ly; ++J)
                for (int I = 0; I < Lx; ++I)
                {
                    const int g = I + Lx * (J + Ly * K), s = I + stride * (J + Ly * K);
                    const double a = h_a ? h_a[g] : 1.0;
                    double h = 0.0;
                    if ((I == 0 && (face_mask & WaveBox::x0)) || (I == Lx - 1 && (face_mask & WaveBox::x1)))
                        h += fx * Wz[K] * Wy[J];
                    if ((J == 0 && (face_mask & WaveBox::y0)) || (J == Ly - 1 && (face_mask & WaveBox::y1)))
                        h += fy * Wz[K] * Wx[I];
                    if ((K == 0 && (face_mask & WaveBox::z0)) || (K == Lz - 1 && (face_mask & WaveBox::z1)))
                        h += fz * Wy[J] * Wx[I];
                    B.m[g] = cm * Wz[K] * Wy[J] * Wx[I];
                    B.h[g] = h;
                    B.invm[g] = 1.0 / (a * a * B.m[g]);
                    B.Hi[g] = h * a;
                    B.slot_of_dof[g] = s;
                    B.dof_of_slot[s] = g;
                }
        return B;
    }
} // namespace cuddh
