// Restarted GMRES(m) on DEVICE vectors.
// Contract: reference include/gmres.hpp:14-36 and the iteration of
// source/gmres.cpp:91-235: r = b - A x; at most maxit-1 restart cycles
// (`for (it = 1; it < maxit; ++it)`); modified Gram-Schmidt; Givens rotations;
// inner exit when |eta_{k+1}| < tol*||b||; true residual after every cycle;
// num_matvec counts every operator application; the preconditioned overload
// applies LEFT preconditioning (solves P A x = P b).
// The Hessenberg column is accumulated on the device and fetched once per
// Arnoldi step instead of one blocking copy per dot product.
#ifndef CUDDH_AMD_KRYLOV_HPP
#define CUDDH_AMD_KRYLOV_HPP

#include <chrono>
#include <iomanip>
#include <iostream>
#include <vector>

#include "blas1.hpp"
#include "operator.hpp"
#include "tensor.hpp"

namespace cuddh
{
    struct solver_out
    {
        bool success;
        int num_iter;
        int num_matvec;
        std::vector<double> res_norm;
        std::vector<double> time;
    };

    solver_out gmres(int n, double *x, const Operator *A, const double *b, const Operator *Precond, int m, int maxit,
                     double tol = 1e-6, int verbose = 0, double max_seconds = 6 * 60 * 60);
    solver_out gmres(int n, double *x, const Operator *A, const double *b, int m, int maxit, double tol = 1e-6,
                     int verbose = 0, double max_seconds = 6 * 60 * 60);
    solver_out gmres(int n, float *x, const SinglePrecisionOperator *A, const float *b, int m, int maxit,
                     float tol = 1e-4, int verbose = 0, double max_seconds = 6 * 60 * 60);

    /// Vectors partitioned over processes (one per GPU): each rank passes its part of x and b (or a copy that is
    /// zero outside the part it owns) and `fn` must sum `count` DEVICE scalars over all ranks in place, ordered on
    /// stream() (an RCCL all-reduce).  Same iteration; every inner product is reduced before it is used, so all
    /// ranks take identical decisions.  Not in the reference (single GPU).
    struct ScalarReduce
    {
        void (*fn)(void *user, void *d_scalars, int count, int is_f64);
        void *user;
    };
    solver_out gmres(int n, double *x, const Operator *A, const double *b, int m, int maxit, double tol, int verbose,
                     double max_seconds, const ScalarReduce &reduce);
    solver_out gmres(int n, float *x, const SinglePrecisionOperator *A, const float *b, int m, int maxit, float tol, int verbose,
                     double max_seconds, const ScalarReduce &reduce);

    /// How an Arnoldi step orthogonalises w = A v_k against v_0..v_k.
    /// mgs (the reference's, the default): modified Gram-Schmidt, one fused launch per basis vector, k + 3 dependent launches.
    /// cgs2: classical Gram-Schmidt applied twice; every coefficient of a pass is an inner product with the same vector, so a pass
    /// is one launch whatever k is: four launches per step, three reductions of k + 1 scalars with partitioned vectors (mgs: k + 2
    /// of one scalar), orthogonality of the basis at working precision.  m <= 512, and with partitioned vectors every rank needs
    /// at least one entry (an error otherwise).  Same iteration otherwise.
    enum class Orthogonalization
    {
        mgs,
        cgs2
    };
    solver_out gmres(int n, double *x, const Operator *A, const double *b, const Operator *Precond, int m, int maxit, double tol, int verbose,
                     double max_seconds, Orthogonalization orth);
    solver_out gmres(int n, double *x, const Operator *A, const double *b, int m, int maxit, double tol, int verbose, double max_seconds,
                     Orthogonalization orth);
    solver_out gmres(int n, float *x, const SinglePrecisionOperator *A, const float *b, int m, int maxit, float tol, int verbose,
                     double max_seconds, Orthogonalization orth);
    solver_out gmres(int n, double *x, const Operator *A, const double *b, int m, int maxit, double tol, int verbose,
                     double max_seconds, const ScalarReduce &reduce, Orthogonalization orth);
    solver_out gmres(int n, float *x, const SinglePrecisionOperator *A, const float *b, int m, int maxit, float tol, int verbose,
                     double max_seconds, const ScalarReduce &reduce, Orthogonalization orth);

    /// Options of the iteration beyond the reference's.
    /// augment = k, 0 <= k < m (an error otherwise; 0, the default, is the iteration above bit for bit): LGMRES (Baker, Jessup and
    /// Manteuffel's "loose GMRES").  The last k corrections z_i = (x_i - x_{i-1}) / |x_i - x_{i-1}| and their images A z_i are kept, most
    /// recent first (2 k vectors beside the m + 1 of the basis), and take the place of the last min(k, stored) columns of every cycle:
    /// a cycle still has at most m columns, columns j < m - ka are Krylov columns (w = A v_j, one operator application), column
    /// m - ka + p searches along z_p with w a copy of A z_p (no operator application, num_matvec unchanged).  w is orthogonalised
    /// and the least-squares problem updated as always, under either orthogonalisation and with partitioned vectors.  At the end of
    /// a cycle dx = sum_j y_j u_j and x <- x + dx in one launch (cuddh_hip_krylov_update_*), and the new pair is dx / |dx| and
    /// (r_old - r_new) / |dx| from the two true residuals the iteration has anyway (none when |dx| = 0).  m <= 512.  Operators that
    /// only queue device work stay driven one step ahead: an augmentation column is a device copy.
    ///
    /// arithmetic = complex (real, the default, is the iteration above bit for bit): the vectors are read as n / 2 complex numbers,
    /// real parts in the first half and imaginary parts in the second (the layout of a DDH trace vector [lambda; mu]), and the
    /// iteration is GMRES(m) over the complex numbers: complex inner products <v, w> = sum conj(v) w, a complex Hessenberg matrix,
    /// complex Givens rotations and coefficients (std::complex<double> on the host whatever the vectors' type).  After j operator
    /// applications the residual is minimised over the COMPLEX combinations of r, A r, .., A^(j-1) r -- twice the real dimensions of the
    /// real iteration -- with the same m + 1 vectors, the same bytes moved and the same launches per Arnoldi step
    /// (cuddh_hip_cmgs_stage_*, cuddh_hip_ckrylov_update_*).  Inner exit, breakdown rule and end of cycle are the real iteration's:
    /// x is updated, the true residual b - A x is formed with the operator and decides.  This assumes that A is complex-linear,
    /// A(i x) = i A(x) with i [a; b] = [-b; a]; where it is so only approximately (DDH with time-stepped local solves: to 4e-3 -- 6e-3
    /// at five WaveHoltz iterations) the estimate inside a cycle is approximate and the true residual still decides.  An operator
    /// that anticommutes with i (HelmholtzOperator: its second row is negated) must stay on real arithmetic.  Where a cycle gains
    /// less than the operator's defect (a stalled GMRES(m)) the true residual may rise from cycle to cycle: res_norm shows it.
    /// Needs an even n, m <= 512, orth = mgs and augment = 0; cgs2, augment > 0, a ScalarReduce or a preconditioner combined with
    /// complex arithmetic is an error.  Operators that only queue device work stay driven one step ahead.
    enum class Arithmetic
    {
        real,
        complex
    };
    struct GmresOptions
    {
        Orthogonalization orth = Orthogonalization::mgs;
        int augment = 0;
        Arithmetic arithmetic = Arithmetic::real;
    };
    solver_out gmres(int n, double *x, const Operator *A, const double *b, const Operator *Precond, int m, int maxit, double tol, int verbose,
                     double max_seconds, const GmresOptions &opt);
    solver_out gmres(int n, double *x, const Operator *A, const double *b, int m, int maxit, double tol, int verbose, double max_seconds,
                     const GmresOptions &opt);
    solver_out gmres(int n, float *x, const SinglePrecisionOperator *A, const float *b, int m, int maxit, float tol, int verbose,
                     double max_seconds, const GmresOptions &opt);
    solver_out gmres(int n, double *x, const Operator *A, const double *b, int m, int maxit, double tol, int verbose,
                     double max_seconds, const ScalarReduce &reduce, const GmresOptions &opt);
    solver_out gmres(int n, float *x, const SinglePrecisionOperator *A, const float *b, int m, int maxit, float tol, int verbose,
                     double max_seconds, const ScalarReduce &reduce, const GmresOptions &opt);
} // namespace cuddh

#endif
