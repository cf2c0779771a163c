// The small problem of GMRES(m): the Hessenberg matrix a cycle builds column by column, the Givens rotations that keep it
// triangular, the rotated right-hand side whose last entry is the residual estimate, and the back substitution that ends the
// cycle.  Host arithmetic only (internal header of krylov.cpp; cuddh_gmres_small_problem runs it without a GPU).
// The entry type is the scalar of the vectors on real arithmetic and std::complex<double> on complex arithmetic
// (krylov.hpp: Arithmetic).  Host code is compiled with contraction inside a statement: every floating-point statement below
// keeps its form, or the last bit of H moves.
#ifndef CUDDH_AMD_GMRES_SMALL_HPP
#define CUDDH_AMD_GMRES_SMALL_HPP

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstddef>
#include <vector>

namespace cuddh
{
    namespace small
    {
        using cplx = std::complex<double>;

        // products and quotients written out (no special-value handling of the library's operators; Smith's division, so that a
        // real divisor divides both parts by it and nothing else)
        inline cplx cmul(cplx a, cplx b) { return {a.real() * b.real() - a.imag() * b.imag(), a.real() * b.imag() + a.imag() * b.real()}; }
        inline cplx cdiv(cplx a, cplx b)
        {
            if (std::abs(b.real()) >= std::abs(b.imag()))
            {
                const double q = b.imag() / b.real(), d = b.real() + b.imag() * q;
                return {(a.real() + a.imag() * q) / d, (a.imag() - a.real() * q) / d};
            }
            const double q = b.real() / b.imag(), d = b.real() * q + b.imag();
            return {(a.real() * q + a.imag()) / d, (a.imag() * q - a.real()) / d};
        }

        // apply the k previous rotations to column h, then build rotation k that zeroes h[k+1]
        template <typename scalar>
        void rotate_column(scalar *h, scalar *cs, scalar *sn, int k)
        {
            for (int i = 0; i < k; ++i)
            {
                const scalar a = h[i], b = h[i + 1];
                h[i] = cs[i] * a + sn[i] * b;
                h[i + 1] = cs[i] * b - sn[i] * a;
            }
            const scalar r = std::hypot(h[k], h[k + 1]);
            cs[k] = h[k] / r;
            sn[k] = h[k + 1] / r;
            h[k] = cs[k] * h[k] + sn[k] * h[k + 1];
            h[k + 1] = 0;
        }

        // the same with complex entries: G_i = [conj(cs_i), conj(sn_i); -sn_i, cs_i], cs_k = h_k / t, sn_k = h_{k+1} / t,
        // t = sqrt(|h_k|^2 + |h_{k+1}|^2) (h_{k+1}, a norm, is real); with real entries these are the operations above
        inline void rotate_column(cplx *h, cplx *cs, cplx *sn, int k)
        {
            for (int i = 0; i < k; ++i)
            {
                const cplx a = h[i], b = h[i + 1];
                h[i] = cmul(std::conj(cs[i]), a) + cmul(std::conj(sn[i]), b);
                h[i + 1] = cmul(cs[i], b) - cmul(sn[i], a);
            }
            const double t = std::hypot(std::hypot(h[k].real(), h[k].imag()), std::hypot(h[k + 1].real(), h[k + 1].imag()));
            cs[k] = {h[k].real() / t, h[k].imag() / t};
            sn[k] = {h[k + 1].real() / t, h[k + 1].imag() / t};
            h[k] = cmul(std::conj(cs[k]), h[k]) + cmul(std::conj(sn[k]), h[k + 1]);
            h[k + 1] = 0;
        }

        // rotation k on the right-hand side; returns the residual estimate |eta_{k+1}|
        template <typename scalar>
        scalar rotate_rhs(scalar *eta, const scalar *cs, const scalar *sn, int k)
        {
            eta[k + 1] = -sn[k] * eta[k];
            eta[k] = cs[k] * eta[k];
            return std::abs(eta[k + 1]);
        }

        inline double rotate_rhs(cplx *eta, const cplx *cs, const cplx *sn, int k)
        {
            eta[k + 1] = -cmul(sn[k], eta[k]);
            eta[k] = cmul(std::conj(cs[k]), eta[k]);
            return std::hypot(eta[k + 1].real(), eta[k + 1].imag());
        }

        // back substitution R y = g for the leading kk x kk block of the (ld x m) column-major array R
        // (the reference calls LAPACK ?trsv('U','N','N'), source/gmres.cpp:26-41)
        template <typename scalar>
        void back_substitute(int kk, const scalar *R, int ld, scalar *g)
        {
            for (int i = kk - 1; i >= 0; --i)
            {
                scalar s = g[i];
                for (int j = i + 1; j < kk; ++j)
                    s -= R[i + ld * j] * g[j];
                g[i] = s / R[i + ld * i];
            }
        }

        inline void back_substitute(int kk, const cplx *R, int ld, cplx *g)
        {
            for (int i = kk - 1; i >= 0; --i)
            {
                cplx sacc = g[i];
                for (int j = i + 1; j < kk; ++j)
                    sacc -= cmul(R[i + static_cast<std::size_t>(ld) * j], g[j]);
                g[i] = cdiv(sacc, R[i + static_cast<std::size_t>(ld) * i]);
            }
        }

        template <typename entry>
        struct real_of
        {
            using type = entry;
        };
        template <>
        struct real_of<cplx>
        {
            using type = double;
        };
    } // namespace small

    /// One GMRES(m) least-squares problem: start a cycle with |r|, push Hessenberg columns, solve for y.
    template <typename entry>
    class GmresSmall
    {
    public:
        using real = typename small::real_of<entry>::type;

        explicit GmresSmall(int m) : m1(m + 1), H(static_cast<std::size_t>(m1) * m, entry(0)), cs(m, entry(0)), sn(m, entry(0)), eta(m1, entry(0)) {}

        void start(real r_nrm)
        {
            std::fill(eta.begin(), eta.end(), entry(0));
            eta[0] = r_nrm;
        }

        /// where column k goes: k + 2 entries, h_0 .. h_k and the norm h_{k+1}
        entry *column(int k) { return H.data() + static_cast<std::size_t>(m1) * k; }

        /// rotates column k (already stored through column(k), h_{k+1} != 0) into the triangle; returns the residual estimate
        real push(int k)
        {
            small::rotate_column(column(k), cs.data(), sn.data(), k);
            return small::rotate_rhs(eta.data(), cs.data(), sn.data(), k);
        }

        /// the coefficients y of the first k1 columns; ends the cycle (the right-hand side is overwritten)
        const entry *solve(int k1)
        {
            small::back_substitute(k1, H.data(), m1, eta.data());
            return eta.data();
        }

    private:
        int m1;
        std::vector<entry> H, cs, sn, eta;
    };

    /// GmresSmall on host arrays, as krylov.cpp compiles it (cuddh_gmres_small_problem): h_cols holds column k as k + 2 entries
    /// (re, im interleaved when complex; float when not f64 and not complex), y_out the ncols coefficients, est_out the estimate
    /// after each column.  Returns false and writes nothing on bad arguments.
    bool gmres_small_problem(int is_complex, int is_f64, int m, int ncols, const void *h_cols, double beta, void *y_out, double *est_out);
} // namespace cuddh

#endif
