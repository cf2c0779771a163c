// Whole-domain WaveHoltz in three dimensions on a box of congruent brick elements: the fixed-point iteration of
// waveholtz.hpp for  (K - w^2 M + i w H) U = f  with the collocated stiffness of the box lattice (wave_box.hpp),
//     K = cx Wz (x) Wy (x) Ax + cy Wz (x) Ay (x) Wx + cz Az (x) Wy (x) Wx,    M = diag(a^2 m),    H = diag(a h),
// m the Gauss-Lobatto lumped mass and h the lumped mass of the absorbing faces (any subset of the six; the others are sound-hard).
// The march is WaveHoltz's lattice form, statement by statement, on csrc/kernels/wave_box.hip: one launch per Runge-Kutta sweep.
// W(z; f) = S z + W(0; f); its fixed point solves (I - S) z = W(0; f); U = u + i v / w.  Call sequence:
//     W.rhs(f, b); gmres(W.size(), z, &W, b, m, maxit, tol); W.solution(z, u);
// Public vectors hold 2 Lx Ly Lz doubles, node (I, J, K) at I + Lx (J + Ly K); all are DEVICE pointers unless marked HOST.
// precision = f32 stores and marches the lattice vectors in fp32 on csrc/kernels/wave_box_f32.hip; the public vectors,
// action and solution stay double.  One launch per sweep, full boxes, beta == 1: the 2-D lattice form's other options (paired
// launches, missing cells, a per-cell stiffness) have no 3-D counterpart yet.
#ifndef CUDDH_AMD_WAVEHOLTZ_BOX_HPP
#define CUDDH_AMD_WAVEHOLTZ_BOX_HPP

#include <string>
#include <vector>

#include "ddh.hpp"
#include "memory.hpp"
#include "operator.hpp"
#include "wave_box.hpp"

namespace cuddh
{
    struct WaveHoltzBoxOptions
    {
        /// rk2 on the mesh grid (the default) or rk4 on ceil(nt_mesh / coarsen) steps, coarsen in [1, 16]: DDHIntegrator's rules
        DDHIntegrator integrator;
        /// the period is time_ratio times the base grid's steps, in [1, DDHTimeStep::max_ratio]; from_coefficient: the ratio is
        /// max(1, ceil((1 - 1e-9) / min a)) over all nodes
        int time_ratio = 1;
        static constexpr int from_coefficient = 0;
        /// the absorbing faces: bits of WaveBox::Face
        unsigned faces = WaveBox::all_faces;
        /// f64 (the default) or f32: the lattice vectors, the stencil and the stages of the march in that precision.  With f32 a
        /// period rounds z_in, f, invm and Hi to float once on the way in (cuddh_hip_wave32_load / _begin) and widens the result on
        /// the way out (_store); rows of the padded lattice hold a multiple of four floats.  nt, dt and the ratio do not depend on it.
        /// fp32 suits GMRES tolerances around 1e-4, not 1e-6.  Any other value is refused
        /// ("WaveHoltz error: precision:").
        enum Precision
        {
            f64,
            f32
        } precision = f64;
    };

    /// The period's grid a WaveHoltzBox of these arguments marches on, from host arithmetic alone (nothing is allocated): every
    /// refusal of the constructor, then nt = ratio * ceil(mesh_grid_steps(omega, min(hx, hy, hz), n_basis) / coarsen), the ratio in
    /// effect and dt = 2 pi / (omega nt).
    struct WaveBoxTimeGrid
    {
        int nt, ratio;
        double dt;
    };
    WaveBoxTimeGrid wave_box_time_grid(double omega, int nx, int ny, int nz, const double *box, int n_basis, const double *h_a,
                                       const WaveHoltzBoxOptions &options);

    class WaveHoltzBox : public Operator
    {
    public:
        /// box = {ax, bx, ay, by, az, bz} (HOST); h_a: HOST coefficient a, one finite positive value per lattice node in public
        /// order.  Anything wave_box.hpp refuses, an omega that is not finite and positive, and an integrator or a ratio outside the
        /// rules above throw before any allocation or launch.
        WaveHoltzBox(double omega, int nx, int ny, int nz, const double *box, int n_basis, const double *h_a, const WaveHoltzBoxOptions &options = {});
        ~WaveHoltzBox();

        WaveHoltzBox(const WaveHoltzBox &) = delete;
        WaveHoltzBox &operator=(const WaveHoltzBox &) = delete;

        /// length of z = [u; v]
        int size() const { return 2 * ndof; }
        /// Lx, Ly, Lz
        void lattice(int dims[3]) const;

        /// z_out = W(z_in; f): one filtered period started from z_in (nullptr: from zero) under the load f = [f_re; f_im]
        /// (nullptr: none, the homogeneous march S z_in).  z_out must not overlap z_in or f.
        void period(const double *z_in, const double *f, double *z_out) const;
        /// b = W(0; f)
        void rhs(const double *f, double *b) const { period(nullptr, f, b); }
        /// u = [z_u; z_v / omega]: real and imaginary part of U.  u may be z.
        void solution(const double *z, double *u) const;

        /// y = x - S x
        void action(const double *x, double *y) const override;
        /// y += c (x - S x)
        void action(double c, const double *x, double *y) const override;

        int num_steps() const { return nt; }
        double time_step() const { return dt; }
        int time_ratio() const { return ratio; }
        DDHIntegrator integrator() const { return scheme; }
        int sweeps_per_period() const { return nt * (scheme.scheme == DDHIntegrator::rk4 ? 4 : 2); }
        /// "wave_box nb<n>", with " f32" at that precision, then " (run-time n_basis)" where n_basis is not a compile-time form of
        /// the kernel file (wave_box.hip: 4; wave_box_f32.hip: 4 and 5)
        std::string stiffness_kernel() const;
        WaveHoltzBoxOptions::Precision precision() const { return f32 ? WaveHoltzBoxOptions::f32 : WaveHoltzBoxOptions::f64; }

    private:
        const double omega;
        WaveBox geo;
        int ndof = 0, slots = 0;
        DDHIntegrator scheme;
        int nt = 0, ratio = 1;
        double dt = 0.0;
        std::vector<double> filt, cs, sn; // HOST tables of the period's grid: filter (nt + 1), cs and sn (2 nt + 1)
        host_device_ivec dof_of_slot, slot_of_dof;
        host_device_dvec invm, Hi; // 1 / (a^2 m) and h a in padded lattice order, zero in the padding
        mutable host_device_dvec p, q, u, v, ps, qs, ps2, aq, ap, F, G, tmp;
        // precision = f32: the lattice vectors as floats (the double ones above, tmp apart, then stay empty)
        bool f32 = false;
        HostDeviceArray<float> invm32, Hi32;
        mutable HostDeviceArray<float> p32, q32, u32, v32, ps32, qs32, ps2_32, aq32, ap32, F32, G32;
    };
} // namespace cuddh

#endif
