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
    struct GmresOptions
    {
        Orthogonalization orth = Orthogonalization::mgs;
        int augment = 0;
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
