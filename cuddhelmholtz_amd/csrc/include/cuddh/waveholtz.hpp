// Whole-domain WaveHoltz: the time-domain fixed-point iteration for  (K - w^2 M + i w H) U = f  on the whole H1Space, with the
// global StiffnessMatrix as the sweep of the march.  M = diag(a^2 m), m the Gauss-Lobatto lumped mass; H = diag(a h)
// on the dofs of the absorbing faces, h the lumped face mass.  The march is the one of the DDH local solves (one subdomain that
// covers the mesh): one period of RK2 or RK4 steps, filtered.  W(z; f) = S z + W(0; f) is affine in z = [u; v], and its fixed
// point solves (I - S) z = W(0; f); U = u + i v / w.  Call sequence:
//     W.rhs(f, b); gmres(W.size(), z, &W, b, m, maxit, tol); W.solution(z, u);
// Its iteration count does not depend on a decomposition; it is NOT a check of DDH's fixed point, which reads the global load in
// every subdomain and is another discrete problem (tests/helmholtz_direct.py).
// sweep = lattice (opt-in; collocated stiffness on a uniform rectangle mesh only): the state lives in lattice order and ONE launch
// per sweep does the stiffness stencil and the stage (csrc/kernels/wave_lattice.hip); no StiffnessMatrix is built.  z, f and
// every public vector keep the space's dof order: a period permutes them in and out.
// A grid mesh with missing cells (meshio.hpp's grid_cells: the cells of a uniform rectangle grid in ascending order, some left
// out) is taken too: where the full-rectangle detection refuses, build_wave_cells_map (wave_lattice.hpp) is tried, and the same
// march runs on csrc/kernels/wave_cells.hip / wave_cells_f32.hip, whose stencil adds up the cells that exist around a node
// (DESIGN 4.5.4).  Lattice nodes with no cell around them are slots without a dof, like padding.  h_faces chooses the walls:
// every boundary edge absorbing (the default) or, with the outer edges only, sound-hard holes.  per_pair is refused there.
// precision = f32 (opt-in; the lattice form only): the march's thirteen lattice vectors are stored and the sweeps computed in
// fp32 (csrc/kernels/wave_lattice_f32.hip), half the march's memory and bytes; z, f, b, the solution and y = x - S x stay fp64,
// rounded once on the way into a period and converted once on the way out.  For tolerances around 1e-4: the fp32 operator's own
// defect is about 1e-6 relative, so a solve to 1e-6 or below wants f64.
// launch = per_pair (opt-in; the lattice form only, both precisions): two sweeps per launch (csrc/kernels/wave_pair.hip and
// wave_pair_f32.hip): rk2_a with rk2_b, rk4_1 with rk4_2 and rk4_3 with rk4_4.  Half the launches, 0.56 x (RK2) and
// 0.48 x (RK4) the vectors moved, and the bits of the per-sweep march.
// h_cell_stiffness (opt-in; the lattice form only, per-sweep launches, both precisions): a coefficient beta per element in the
// stiffness,  -div(beta grad U) - w^2 a^2 U = f  (csrc/kernels/wave_weights.hip and wave_weights_f32.hip).  M and H
// keep their form, so the absorbing faces discretise  beta dU/dn + i w a U = 0:  the first-order absorbing condition only where
// beta = 1 along them.
// Everything else is fp64; all vectors are DEVICE pointers unless marked HOST.
#ifndef CUDDH_AMD_WAVEHOLTZ_HPP
#define CUDDH_AMD_WAVEHOLTZ_HPP

#include <memory>
#include <string>
#include <vector>

#include "ddh.hpp"
#include "memory.hpp"
#include "operator.hpp"
#include "operators.hpp"
#include "spaces.hpp"

namespace cuddh
{
    struct WaveHoltzOptions
    {
        /// rk2 on the mesh grid (the default) or rk4 on ceil(nt_mesh / coarsen) steps, coarsen in [1, 16]: DDHIntegrator's rules
        DDHIntegrator integrator;
        /// the period is time_ratio times the base grid's steps, in [1, DDHTimeStep::max_ratio]; from_coefficient: the ratio is
        /// max(1, ceil((1 - 1e-9) / min a)) over all dofs
        int time_ratio = 1;
        static constexpr int from_coefficient = 0;
        /// gauss: StiffnessMatrix(fem) (n_basis + 1 Gauss-Legendre points, the plan kernels); lobatto: the n_basis-point Gauss-Lobatto
        /// rule, the collocated stiffness of the DDH local solves, on whatever kernel StiffnessMatrix runs it
        enum Stiffness
        {
            gauss,
            lobatto
        };
        Stiffness stiffness = gauss;
        /// operator_kernels (the default): a stiffness apply and a stage kernel per sweep.  lattice: one launch per sweep on
        /// lattice-ordered vectors; needs stiffness = lobatto and a uniform rectangle mesh (detected: cuddh/wave_lattice.hpp),
        /// anything else is refused ("WaveHoltz error: sweep: ...") before any allocation
        enum Sweep
        {
            operator_kernels,
            lattice
        };
        Sweep sweep = operator_kernels;
        /// f64 (the default) or f32: the lattice vectors and sweeps in fp32.  f32 needs sweep = lattice; anything else is refused
        /// ("WaveHoltz error: precision: ...") before any allocation or launch
        enum Precision
        {
            f64,
            f32
        };
        Precision precision = f64;
        /// per_sweep (the default): one launch per sweep.  per_pair: two sweeps of the lattice form per launch, bit for bit the same
        /// march.  per_pair needs sweep = lattice; anything else is refused ("WaveHoltz error: launch: ...") before any allocation
        enum Launch
        {
            per_sweep,
            per_pair
        };
        Launch launch = per_sweep;
        /// absorbing faces: HOST edge ids; n_faces < 0 (the default): every boundary edge, DDH's choice
        const int *h_faces = nullptr;
        int n_faces = -1;
        /// a per-cell stiffness coefficient beta (HOST, n_elem values in element order, each finite and positive; nullptr, the
        /// default: beta == 1 and exactly the code paths above): the problem becomes  -div(beta grad U) - w^2 a^2 U = f  with beta
        /// constant on each element.  It needs sweep = lattice and runs csrc/kernels/wave_weights.hip /
        /// wave_weights_f32.hip on full rectangles and on grids with missing cells alike; a bad value or another sweep is refused
        /// ("WaveHoltz error: cell_stiffness: ..."), launch = per_pair with it too ("WaveHoltz error: launch: ..."), before any
        /// allocation or launch.  from_coefficient then is max(1, ceil((1 - 1e-9) max_e (sqrt(beta_e) / min_{g in e} a_g))).
        /// Mass and faces are unchanged, M = diag(a^2 m) and H = diag(a h): the boundary condition discretised is
        /// beta dU/dn + i w a U = 0, the first-order absorbing condition only where beta = 1 along the absorbing faces.
        const double *h_cell_stiffness = nullptr;
    };

    class WaveHoltz : public Operator
    {
    public:
        /// h_a: HOST nodal coefficient a(x), finite and positive (anything else throws before any allocation or launch, as do an
        /// integrator or a ratio outside the rules above)
        WaveHoltz(double omega, const double *h_a, const H1Space &fem, const WaveHoltzOptions &options = {});
        ~WaveHoltz();

        WaveHoltz(const WaveHoltz &) = delete;
        WaveHoltz &operator=(const WaveHoltz &) = delete;

        /// length of z = [u; v]
        int size() const { return 2 * ndof; }

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
        /// kernel the stiffness sweep launches (after the first period; "generic" = element_ops.hip); the lattice form names its
        /// kernel and n_basis
        std::string stiffness_kernel() const;
        WaveHoltzOptions::Sweep sweep() const { return lat ? WaveHoltzOptions::lattice : WaveHoltzOptions::operator_kernels; }
        WaveHoltzOptions::Precision precision() const;
        WaveHoltzOptions::Launch launch() const;

    private:
        struct Lattice; // the lattice form's description, maps and second ps; in fp32 all its vectors (waveholtz.cpp)
        void lattice_period(const double *z_in, const double *f, double *z_out) const;

        const double omega;
        const int ndof;
        DDHIntegrator scheme;
        int nt = 0, ratio = 1;
        double dt = 0.0;
        std::vector<double> filt, cs, sn; // HOST tables of the period's grid: filter (nt + 1), cs and sn (2 nt + 1)
        std::unique_ptr<StiffnessMatrix> K; // null in the lattice form
        std::unique_ptr<Lattice> lat;       // null in the operator form
        host_device_dvec invm, Hi;        // 1 / (a^2 m) and h a (zero off the absorbing faces), ndof each (lattice form: its slots)
        // the march's state and stage vectors (each 16-byte aligned whatever ndof is, so that the stages take their 16-byte path);
        // all but tmp stay empty in the fp32 lattice form
        mutable host_device_dvec w, p, q, u, v, ps, qs, aq, ap, F, G, tmp;
    };
} // namespace cuddh

#endif
