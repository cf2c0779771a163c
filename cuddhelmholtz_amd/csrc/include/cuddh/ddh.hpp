// Substructured domain-decomposition Helmholtz solver (WaveHoltz local solves).
// Contract: reference include/DDH.hpp:21-84.  Call sequence
// (reference examples/DDH.cpp:141-144):  F.rhs(f, b); gmres(F.size(), lambda, &F, b, ...);
// F.postprocess(lambda, f, u).  `action` applies I - T to the interface traces.
//
// DDH works in fp32 like the reference.  DDH64 is the same algorithm in fp64
// with double traces; it exists so parity against the fp64 oracle can be gated
// at 1e-10 (the reference's float LDS atomics make its own results
// order-dependent, source/DDH.cpp:108).
#ifndef CUDDH_AMD_DDH_HPP
#define CUDDH_AMD_DDH_HPP

#include <memory>
#include <vector>

#include "blas1.hpp"
#include "ensemble.hpp"
#include "krylov.hpp"
#include "memory.hpp"
#include "operator.hpp"
#include "operators.hpp"

struct cuddh_ddh_plan;

namespace cuddh
{
    /// tag of the constructors that take subdomains as element labels: DDH(from_labels, omega, h_a, fem, n_domains, labels)
    struct from_labels_t
    {
        explicit constexpr from_labels_t() = default;
    };
    inline constexpr from_labels_t from_labels{};

    /// Where the local solves take their time step from (block-grid constructors, and the label constructors that take one).
    /// The mesh grid is the reference's: dt = 0.1 h / n_basis^2 shrunk so that nt steps are one period, whatever the
    /// coefficient.  The wave speed is 1 / a, so where a < 1 that step is too long for the explicit time stepping.
    /// Subdomain s may instead march r_s nt steps of dt / r_s, r_s an integer >= 1: local solves couple through the traces
    /// only, so every subdomain runs its own period on its own grid.
    struct DDHTimeStep
    {
        enum Policy
        {
            mesh,        ///< one grid from the mesh alone: the default, the reference's
            coefficient, ///< r_s = max(1, ceil((1 - 1e-9) / min a over the subdomain's dofs)), interface dofs included; a >= 1 gives 1
            ratios       ///< r_s = h_ratios[s]
        };
        Policy policy = mesh;
        const int *h_ratios = nullptr; ///< `ratios`: HOST, one per subdomain, each in [1, max_ratio]; read by the constructor only
        int n_ratios = 0;              ///< must be the number of subdomains
        static constexpr int max_ratio = 256;

        static DDHTimeStep from_mesh() { return {}; }
        static DDHTimeStep from_coefficient() { return {coefficient, nullptr, 0}; }
        static DDHTimeStep from_ratios(const int *h_ratios, int n) { return {ratios, h_ratios, n}; }
    };

    /// How the local solves step in time, and on how coarse a grid (block-grid constructors, and the label constructors that take one).
    /// rk2: the reference's explicit midpoint rule on the reference's grid, two stiffness sweeps per step; the default.
    /// rk4: classical Runge-Kutta, four sweeps per step, on a base grid of ceil(nt_mesh / coarsen) steps, nt_mesh the mesh
    /// grid's; a DDHTimeStep ratio r_s multiplies that count as it multiplies the mesh grid's.  The mesh grid is as fine as it
    /// is because the midpoint rule amplifies every undamped mode by 1 + (mu dt)^4 / 8 per step, not for
    /// accuracy: RK4 at coarsen 4 is closer to the exact local solve than RK2 on the mesh grid, in half the sweeps.
    /// Stable range: with a == 1 the largest eigenvalue of a subdomain's first-order system times the mesh step is 0.12
    /// against RK4's 2.78, so the range ends near coarsen 23; max_coarsen = 16 keeps a margin.  The range scales with min a
    /// over a subdomain unless DDHTimeStep::coefficient compensates: with a = 0.2 and the mesh policy, coarsen <= 4.
    struct DDHIntegrator
    {
        enum Scheme
        {
            rk2,
            rk4
        };
        Scheme scheme = rk2;
        int coarsen = 1; ///< in [1, max_coarsen]; rk2 takes 1 only, so that an rk2 plan is exactly what it was
        static constexpr int max_coarsen = 16;

        static DDHIntegrator rk4_on(int coarsen = 4) { return {rk4, coarsen}; }
    };

    namespace detail
    {
        /// setup shared by DDH and DDH64 (scalar = float or double)
        template <typename Real>
        class DDHCore
        {
        public:
            DDHCore(double omega, const double *h_a, const H1Space &fem, int nx, int ny, int kernel);
            /// block x block elements per subdomain: 0 or 16 / n_basis is the size of the constructor above; else block >= 1 with
            /// n_basis^2 block^2 <= 1024 and nx, ny multiples of block (anything else throws before any allocation or launch)
            DDHCore(double omega, const double *h_a, const H1Space &fem, int nx, int ny, int kernel, int block);
            /// the same with a time-step policy.  `coefficient` with ONE ratio r for all subdomains is a plain plan on the grid of
            /// r nt steps (a == 1 everywhere: the constructor above, bit for bit); several ratios, and `ratios` always, give a plan
            /// with per-subdomain time grids (cuddh_hip_ddh_plan_set_time_grids).  A non-finite or non-positive a, a ratio outside
            /// [1, 256] and a ratio array of the wrong length throw before any allocation or launch.
            DDHCore(double omega, const double *h_a, const H1Space &fem, int nx, int ny, int kernel, int block, const DDHTimeStep &time_step);
            /// the same with an integrator.  An unknown scheme, a coarsen outside [1, 16] and coarsen > 1 with rk2 throw before any
            /// allocation or launch; a kernel that has no RK4 form (cuddh_hip_ddh_plan_set_integrator) throws on first use.
            DDHCore(double omega, const double *h_a, const H1Space &fem, int nx, int ny, int kernel, int block, const DDHTimeStep &time_step,
                    const DDHIntegrator &integrator);
            /// subdomain s = the elements with label s (HOST, one per element, in [0, n_domains)); any connectivity.
            /// kernel: 0 auto, 9 or 10 (cuddh_hip_ddh_plan_create_general)
            DDHCore(from_labels_t, double omega, const double *h_a, const H1Space &fem, int n_domains, const int *labels, int kernel);
            /// the same with a time-step policy and an integrator, which mean what they mean on the block grid (ratios: one per
            /// label).  Checked in this order, on the host, before any allocation or launch: the integrator, the labels, the policy.
            /// Kernels 9 and 10 both have every form, so nothing about the kernel is refused that the constructor above accepts.
            DDHCore(from_labels_t, double omega, const double *h_a, const H1Space &fem, int n_domains, const int *labels, int kernel,
                    const DDHTimeStep &time_step, const DDHIntegrator &integrator);
            ~DDHCore();

            int n_traces() const { return 2 * n_lambda; }
            int num_domains() const { return n_domains; }
            /// the base grid: the mesh grid (coarsened by the integrator's factor), or under `coefficient` with one ratio r for all
            /// subdomains the grid of r times its steps
            int num_steps() const { return nt; }
            double time_step() const { return dt; }
            /// steps of subdomain s = time_ratios()[s] * mesh_steps(); with an integrator that coarsens, ceil(mesh grid's / coarsen)
            int mesh_steps() const;
            DDHIntegrator integrator() const;
            const std::vector<int> &time_ratios() const;
            /// distinct ratios of a plan with per-subdomain time grids, ascending; empty for a plan on the base grid alone
            const std::vector<int> &time_grid_ratios() const;
            /// HOST tables of the grid of `ratio` * mesh_steps() steps: which = 0 filter, 1 cs, 2 sn.  Returns the length (0: no such grid)
            long long time_grid_table(int ratio, int which, const Real *&table) const;
            int kernel_kind() const;
            /// WaveHoltz iterations per local solve; the reference hard-wires 5 (source/DDH.cpp:136), the default.
            /// Verification knob (tests/test_ddh_physics.py), see cuddh_hip_ddh_plan_set_wh_iters.
            void set_waveholtz_iterations(int n) const;
            /// The wavefronts of the following solve() calls take issue priority over other resident work (s_setprio): for the
            /// multi-GPU schedule that runs the subdomains other ranks wait for beside the rest (cuddh_hip_ddh_plan_set_wave_priority).
            void set_wave_priority(bool high) const;
            /// Kernel 5's sweep form: 0 auto, 1 matrix, 2 element-lane, 3 the same with the other owner rule (cuddh_hip_ddh_plan_set_sweep_form; a form the plan
            /// cannot take throws).  sweep_form() returns the form in effect.
            void set_sweep_form(int form) const;
            int sweep_form() const;
            /// The summation order of the element-lane form's in-lane products: 0 auto, 1 pinned (the chains of the node-by-node loop, bit for bit),
            /// 2 paired (both halves of a register pair meet every term at the same place: 7 packed instructions per pair instead of 8.9;
            /// cuddh_hip_ddh_plan_set_chain_order; an order the plan cannot take throws).  Auto is paired where auto chose the element-lane form
            /// and pinned where set_sweep_form forced it.  chain_order() returns the order in effect, 0 where that form is not.
            void set_chain_order(int order) const;
            int chain_order() const;
            /// Where the element-lane form's march applies the trace sources: 0 auto, 1 in every WaveHoltz pass, 2 in the first pass only (the
            /// later passes run a time loop without source terms and add the first pass's result; beside the paired chains only;
            /// cuddh_hip_ddh_plan_set_forcing; a value the plan cannot take throws).  Auto is 2 where form and order are auto too and auto
            /// gave the paired chains.  forcing() returns the forcing in effect, 0 where the paired chains are not.
            void set_forcing(int forcing) const;
            int forcing() const;
            /// How that march carries the velocity: 0 auto, 1 as it is, 2 scaled by 1 / (2 hm) with its midpoint update folded into the
            /// sweep (beside forcing 2 only; cuddh_hip_ddh_plan_set_march; a value the plan cannot take throws).  Auto is 2 where form,
            /// order and forcing are auto too and auto gave forcing 2.  march() returns the march in effect, 0 where forcing 2 is not.
            void set_march(int march) const;
            int march() const;
            /// What march 2 carries as the velocity: 0 auto, 1 q / (2 hm), 2 that times the head coefficient of the first sweep's chain,
            /// so that the chain opens on the state (cuddh_hip_ddh_plan_set_head; a value the plan cannot take throws).  Auto is 2
            /// wherever the march in effect is 2.  head() returns the head in effect, 0 where march 2 is not.
            void set_head(int head) const;
            int head() const;
            /// How head 2 forms the neighbour sums of its sweeps: 0 auto, 1 DPP on the vector pipe (one copy of a shared node forms the
            /// sum, the other takes it), 2 every copy fetches the other's partial sum over the LDS pipe and adds it itself, bit for bit
            /// the same results (cuddh_hip_ddh_plan_set_assembly; 2 throws where head 2 is not in effect).  assembly() returns the
            /// assembly in effect, 0 where head 2 is not.
            void set_assembly(int assembly) const;
            int assembly() const;
            /// The owner rule of kernels 11, 12 and 13: which copy of a node shared by 2 or 4 elements publishes (false: the first, the default;
            /// true: the last).  A check that the copies are bitwise equal (cuddh_hip_ddh_plan_set_owner_rule); other kernels throw.
            void set_last_copy_publishes(bool last) const;
            const EnsembleSpace &ensemble() const { return *efem; }

            /// runs the local solves of subdomains [dom_begin, dom_end)
            void solve(int dom_begin, int dom_end, const double *x, double *y, bool zero_y, const Real *lambda,
                       Real *update) const;
            /// traces only, for the n subdomains listed in d_domains (DEVICE), one launch (cuddh_hip_ddh_apply_list_*)
            void solve_listed(const int *d_domains, int n, const double *x, const Real *lambda, Real *update) const;
            /// the general form for listed subdomains (solution output y as in solve())
            void solve_listed(const int *d_domains, int n, const double *x, double *y, bool zero_y, const Real *lambda, Real *update) const;

            // host copies of the constructor's tables (tests compare them with the oracle)
            const host_device_ivec &table_B() const { return _Bf; }
            const host_device_ivec &table_gI() const { return _gI; }
            const host_device_ivec &table_sI() const { return _sI; }
            const HostDeviceArray<Real> &table_D() const { return _D; }
            const HostDeviceArray<Real> &table_G() const
            {
                ensure_plan();
                return _g_tensor;
            }
            const HostDeviceArray<Real> &table_m() const { return _m; }
            const HostDeviceArray<Real> &table_gmi() const { return _gmi; }
            const HostDeviceArray<Real> &table_a() const { return _a; }
            const HostDeviceArray<Real> &table_H() const { return _H; }
            const HostDeviceArray<Real> &table_filter() const { return _wh_filter; }
            const HostDeviceArray<Real> &table_cs() const { return _cs; }
            const HostDeviceArray<Real> &table_sn() const { return _sn; }
            int max_dof() const { return mx_dof; }
            int max_fdof() const { return mx_fdof; }
            /// elements per block side in effect; 0 for subdomains built from labels
            int elems_per_side() const { return nel1d; }
            bool label_built() const { return general; }

        private:
            /// everything after the element labels (time grid, slots, renumbering, masses, H, a)
            void setup(const double *h_a, const H1Space &fem, const int *labels, const DDHTimeStep &time_step);
            /// the integrator into `more`, or an error
            void set_integrator(const DDHIntegrator &integrator);
            /// nel1d from `block` (0: 16 / n_basis), or an error: n_basis, block and the divisibility of nx, ny
            void set_block(int nx, int ny, int block);
            /// the block grid's element labels, then setup()
            void setup_blocks(const double *h_a, const H1Space &fem, int nx, int ny, const DDHTimeStep &time_step = {});
            /// the time grid(s) and their tables; needs gI
            void setup_time_grids(const double *h_a, const H1Space &fem, const DDHTimeStep &time_step);
            void solve_impl(const int *d_list, int d0, int d1, const double *x, double *y, bool zero_y, const Real *lambda, Real *update) const;

            /// device-side part of the set-up (geometric factors, kernel plan); deferred to first use so
            /// that the host tables can be built and inspected without a GPU
            void ensure_plan() const;
            /// tables of the fixed-order assembly of y (first call with y != nullptr)
            void ensure_assembly() const;

            int g_ndof, g_elem, n_basis, n_domains, n_lambda, nt, mx_dof, mx_fdof, mx_elem_per_dom, nel1d;
            double omega, dt;
            const Mesh2D *fem_mesh;
            /// The time grids' state (and the basis) behind one pointer, in the place the basis pointer had: the size of DDH /
            /// DDH64 and the offsets of what the inline accessors read stay what they were, so a program compiled against the
            /// header as it was before the time-step policy (a drop-in driver built once, say) runs with this library.
            struct More;
            std::unique_ptr<More> more;
            int requested_kernel = 0;
            bool general = false; // subdomains from labels: cuddh_hip_ddh_plan_create_general

            host_device_ivec _Bf, _gI, _sI;
            HostDeviceArray<Real> _D, _m, _gmi, _H, _wh_filter, _cs, _sn, _a;
            mutable HostDeviceArray<Real> _g_tensor;
            std::unique_ptr<EnsembleSpace> efem;
            mutable cuddh_ddh_plan *plan = nullptr;
            // y = sum over subdomains of weighted local solutions, assembled in a fixed order instead of with atomics:
            // identity numbering of the subdomain dofs, their forcing / solution in that numbering, and per global dof the
            // list of subdomain dofs that are copies of it (increasing subdomain, like the reference's serial meaning)
            mutable host_device_ivec _gI_local, _csr_off, _csr_src;
            mutable host_device_dvec _x_local, _y_local;
        };
    } // namespace detail

    class DDH : public SinglePrecisionOperator
    {
    public:
        /// @param h_a HOST nodal coefficient a(x); @param fem space on a Mesh2D::uniform_rect(nx, ..., ny, ...) mesh
        DDH(double omega, const double *h_a, const H1Space &fem, int nx, int ny);
        /// extension: pick the local-solve kernel (0 auto, 1 generic workgroup, 2 wavefront-per-subdomain, 3-7 the fp32 forms of
        /// cuddh_hip_ddh_plan_create; 8 is fp64 only, see DDH64).  A requested kernel that does not apply throws on first use.
        DDH(double omega, const double *h_a, const H1Space &fem, int nx, int ny, int kernel);
        /// extension: subdomains of block x block elements (0 or 16 / n_basis: the size of the constructors above).  Needs
        /// block >= 1, n_basis^2 block^2 <= 1024, nx and ny multiples of block; throws otherwise.  kernel: 0 auto, 1 generic
        /// workgroup (any block), 11 one 8 x 8 block per wavefront (n_basis 4, block 8, fp32), 12 four 4 x 4 blocks per wavefront
        /// with one element per lane (n_basis 5, block 4, fp32, rectangles, one time grid, RK2), 13 (on request only) the
        /// element-lane local solves with four 4 x 4 blocks per wavefront at n_basis 4 or 5 (block 4, fp32, rectangles, RK2) that
        /// take any DDHTimeStep: a wavefront marches once per distinct time grid among its four subdomains; 2-8 on their own
        /// block size only.
        DDH(double omega, const double *h_a, const H1Space &fem, int nx, int ny, int kernel, int block);
        /// extension: the same with a time-step policy (DDHTimeStep: from the mesh, from the coefficient, or given per subdomain)
        DDH(double omega, const double *h_a, const H1Space &fem, int nx, int ny, int kernel, int block, const DDHTimeStep &time_step);
        /// extension: the same with an integrator (DDHIntegrator: the reference's RK2, or RK4 on a coarser grid)
        DDH(double omega, const double *h_a, const H1Space &fem, int nx, int ny, int kernel, int block, const DDHTimeStep &time_step,
            const DDHIntegrator &integrator);
        /// extension: subdomains of any shape on any Mesh2D, given as element labels (HOST, n_elem of them, in [0, n_domains),
        /// every subdomain non-empty and with at most 256 element nodes).  kernel: 0 auto, 9 one wavefront per subdomain
        /// (n_basis 4, <= 16 elements per subdomain), 10 one workgroup per subdomain.  Invalid labels throw here.
        DDH(from_labels_t, double omega, const double *h_a, const H1Space &fem, int n_domains, const int *labels, int kernel = 0);
        /// extension: the same with a time-step policy (ratios: one per label) and an integrator; the constructor above is
        /// DDHTimeStep::from_mesh() and RK2
        DDH(from_labels_t, double omega, const double *h_a, const H1Space &fem, int n_domains, const int *labels, int kernel,
            const DDHTimeStep &time_step, const DDHIntegrator &integrator);
        ~DDH() = default;

        /// dimension of the substructured problem
        int size() const { return core.n_traces(); }

        void rhs(const double *f, float *b) const;
        void postprocess(const float *lambda, const double *f, double *u) const;
        void action(const float *x, float *y) const override;

        /// extension for the multi-GPU path: update <- T_local(lambda) over subdomains [d0, d1) only
        /// (slots written by other subdomains are left untouched); no `lambda - update` step.
        void local_traces(int d0, int d1, const double *f, const float *lambda, float *update) const;
        void local_solution(int d0, int d1, const float *lambda, const double *f, double *u, bool zero_u) const;

        const detail::DDHCore<float> &internals() const { return core; }

    private:
        detail::DDHCore<float> core;
    };

    class DDH64 : public Operator
    {
    public:
        /// kernel: 0 auto (3 for n_basis 4), 1 generic, 2 wavefront-per-subdomain, 6 n_basis 8, 8 = the dense element matrix on
        /// the fp64 matrix cores (n_basis 4, uniform metric; on request only).  See cuddh_hip_ddh_plan_create.
        DDH64(double omega, const double *h_a, const H1Space &fem, int nx, int ny, int kernel = 0);
        /// subdomains of block x block elements, as DDH(..., kernel, block); kernel 0 or 1 off the default block size
        DDH64(double omega, const double *h_a, const H1Space &fem, int nx, int ny, int kernel, int block);
        DDH64(double omega, const double *h_a, const H1Space &fem, int nx, int ny, int kernel, int block, const DDHTimeStep &time_step);
        DDH64(double omega, const double *h_a, const H1Space &fem, int nx, int ny, int kernel, int block, const DDHTimeStep &time_step,
              const DDHIntegrator &integrator);
        /// subdomains from element labels, as DDH(from_labels, ...)
        DDH64(from_labels_t, double omega, const double *h_a, const H1Space &fem, int n_domains, const int *labels, int kernel = 0);
        DDH64(from_labels_t, double omega, const double *h_a, const H1Space &fem, int n_domains, const int *labels, int kernel,
              const DDHTimeStep &time_step, const DDHIntegrator &integrator);

        int size() const { return core.n_traces(); }

        void rhs(const double *f, double *b) const;
        void postprocess(const double *lambda, const double *f, double *u) const;
        void action(const double *x, double *y) const override;
        /// not defined for the substructured operator
        void action(double c, const double *x, double *y) const override;

        void local_traces(int d0, int d1, const double *f, const double *lambda, double *update) const;
        void local_solution(int d0, int d1, const double *lambda, const double *f, double *u, bool zero_u) const;

        const detail::DDHCore<double> &internals() const { return core; }

    private:
        detail::DDHCore<double> core;
    };
} // namespace cuddh

#endif
