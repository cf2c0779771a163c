// The small problem of GMRES (csrc/src/gmres_small.hpp) as a stand-alone host program, for a sanitizer run on the CPU:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Icuddhelmholtz_amd/csrc/src \
//       profiles/tools/gmres_small_sanitized.cpp -o /tmp/gmres_small_sanitized && /tmp/gmres_small_sanitized
// The cases of tests/test_gmres_small_problem.py's shapes: m in {1, 2, 5}, ncols in {1, m}, float, double and complex entries, a
// dominant diagonal and a positive subdiagonal.  Each run checks the estimate of the last column against |beta e_1 - H y| formed
// directly, and complex entries with zero imaginary parts against the real path.  Exit status 0 and "ok" when all agree.
#include <cstdio>
#include <cstdlib>

#include "gmres_small.hpp"

using cuddh::GmresSmall;
using cplx = std::complex<double>;

static unsigned long long state = 12345;
static double uniform(double lo, double hi)
{
    state = state * 6364136223846793005ULL + 1442695040888963407ULL;
    return lo + (hi - lo) * static_cast<double>(state >> 11) / 9007199254740992.0;
}

template <typename entry>
static entry off_diagonal()
{
    if constexpr (sizeof(entry) == sizeof(cplx))
        return entry(uniform(-0.4, 0.4), uniform(-0.4, 0.4));
    else
        return static_cast<entry>(uniform(-0.4, 0.4));
}

// runs one problem; returns |estimate - directly formed residual| / beta and leaves y in y_out
template <typename entry>
static double run(int m, int ncols, const std::vector<std::vector<entry>> &cols, double beta, std::vector<entry> &y_out)
{
    GmresSmall<entry> lsq(m);
    lsq.start(static_cast<typename GmresSmall<entry>::real>(beta));
    double est = 0;
    for (int k = 0; k < ncols; ++k)
    {
        std::copy(cols[k].begin(), cols[k].end(), lsq.column(k));
        est = static_cast<double>(lsq.push(k));
    }
    const entry *y = lsq.solve(ncols);
    y_out.assign(y, y + ncols);
    double rr = 0;
    for (int i = 0; i <= ncols; ++i)
    {
        cplx r = i == 0 ? beta : 0.0;
        for (int k = (i > 0 ? i - 1 : 0); k < ncols; ++k)
            r -= cplx(cols[k][i]) * cplx(y_out[k]);
        rr += std::norm(r);
    }
    return std::abs(est - std::sqrt(rr)) / beta;
}

template <typename entry>
static std::vector<std::vector<entry>> columns(int ncols)
{
    std::vector<std::vector<entry>> cols(ncols);
    for (int k = 0; k < ncols; ++k)
    {
        for (int j = 0; j < k; ++j)
            cols[k].push_back(off_diagonal<entry>());
        cols[k].push_back(static_cast<entry>(uniform(1.0, 1.5)));
        cols[k].push_back(static_cast<entry>(uniform(0.2, 0.6)));
    }
    return cols;
}

int main()
{
    int bad = 0;
    const double beta = 1.75;
    for (int m : {1, 2, 5})
        for (int ncols : {1, m})
        {
            std::vector<float> yf;
            std::vector<double> yd;
            std::vector<cplx> yc, yr;
            const double ef = run<float>(m, ncols, columns<float>(ncols), beta, yf);
            const auto cd = columns<double>(ncols);
            const double ed = run<double>(m, ncols, cd, beta, yd);
            const double ec = run<cplx>(m, ncols, columns<cplx>(ncols), beta, yc);
            std::vector<std::vector<cplx>> real_as_complex(ncols);
            for (int k = 0; k < ncols; ++k)
                real_as_complex[k].assign(cd[k].begin(), cd[k].end());
            run<cplx>(m, ncols, real_as_complex, beta, yr);
            double dist = 0;
            for (int k = 0; k < ncols; ++k)
                dist = std::max(dist, std::abs(yr[k] - yd[k]) / std::abs(yd[k]));
            std::printf("m %d ncols %d: estimate off by %.2e (float) %.2e (double) %.2e (complex) of beta; complex with real entries %.2e from real\n", m, ncols,
                        ef, ed, ec, dist);
            bad += !(ef < 1e-4 && ed < 1e-12 && ec < 1e-12 && dist < 1e-12);
        }
    std::puts(bad ? "MISMATCH" : "ok");
    return bad ? EXIT_FAILURE : EXIT_SUCCESS;
}
