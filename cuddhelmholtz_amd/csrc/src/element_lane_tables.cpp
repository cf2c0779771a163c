// Tables of the separable DDH sweeps: see kernels/element_lane_tables.hpp.  Plain C++: nothing here touches the device.
#include "element_lane_tables.hpp"

#include <algorithm>
#include <cmath>

#include "cuddh_hip.h"

namespace cuddh_k
{
    template <int NB>
    int separable_factors(const float *hD, const float *hG, double (&Ax)[NB][NB], double (&Ay)[NB][NB], double (&beta)[NB], double (&gamma)[NB])
    {
        constexpr int NN = NB * NB;
        auto Dm = [&](int a, int b) { return static_cast<double>(hD[a + NB * b]); }; // D(a,b)
        auto g = [&](int c, int k, int l) { return static_cast<double>(hG[3 * (k + NB * l) + c]); };
        double scale = 0.0;
        for (int n = 0; n < NN; ++n)
            scale = std::max(scale, std::fabs(static_cast<double>(hG[3 * n])) + std::fabs(static_cast<double>(hG[3 * n + 2])));
        double alpha[NB], delta[NB];
        for (int i = 0; i < NB; ++i)
        {
            alpha[i] = g(0, i, 0);
            beta[i] = g(0, 0, i) / g(0, 0, 0);
            gamma[i] = g(2, i, 0) / g(2, 0, 0);
            delta[i] = g(2, 0, i);
        }
        for (int l = 0; l < NB; ++l)
            for (int k = 0; k < NB; ++k)
                if (std::fabs(g(1, k, l)) > 1e-6 * scale || std::fabs(g(0, k, l) - alpha[k] * beta[l]) > 1e-6 * scale ||
                    std::fabs(g(2, k, l) - gamma[k] * delta[l]) > 1e-6 * scale)
                    return -1;
        for (int a = 0; a < NB; ++a)
            for (int b = 0; b < NB; ++b)
            {
                double ax = 0.0, ay = 0.0;
                for (int i = 0; i < NB; ++i)
                {
                    ax += Dm(i, a) * alpha[i] * Dm(i, b);
                    ay += Dm(i, a) * delta[i] * Dm(i, b);
                }
                Ax[a][b] = ax;
                Ay[a][b] = ay;
            }
        return 0;
    }

    template <int NB>
    int element_lane_tables(const float *hD, const float *hG, float *out)
    {
        constexpr int NN = NB * NB, LAST = NB - 1;
        double Ax[NB][NB], Ay[NB][NB], beta[NB], gamma[NB];
        if (const int c = separable_factors<NB>(hD, hG, Ax, Ay, beta, gamma))
            return c;
        double W[NB][NB], wmax = 0.0;
        for (int k = 0; k < NB; ++k)
            for (int l = 0; l < NB; ++l)
            {
                W[k][l] = gamma[k] * beta[l];
                if (!(W[k][l] > 0.0) || !std::isfinite(W[k][l]))
                    return -1;
                wmax = std::max(wmax, W[k][l]);
            }
        for (int i = 0; i < NB; ++i)
            if (!(std::fabs(W[LAST][i] - W[0][i]) <= 1e-6 * wmax) || !(std::fabs(W[i][LAST] - W[i][0]) <= 1e-6 * wmax))
                return -1;
        float hS[5 * NN];
        for (int a = 0; a < NB; ++a)
            for (int b = 0; b < NB; ++b)
            {
                const double bx = Ax[a][b] / gamma[a], by = Ay[a][b] / beta[a];
                hS[a + NB * b] = static_cast<float>(bx);
                hS[NN + a + NB * b] = static_cast<float>(by);
                hS[2 * NN + a + NB * b] = static_cast<float>(Ax[a][a] / gamma[a] + Ay[b][b] / beta[b]);
                const double w = W[a == LAST ? 0 : a][b == LAST ? 0 : b];
                hS[3 * NN + a + NB * b] = static_cast<float>(w);
                hS[4 * NN + a + NB * b] = static_cast<float>(1.0 / w);
            }
        for (int i = 0; i < 5 * NN; ++i)
            if (!std::isfinite(hS[i]))
                return -1;
        std::copy(hS, hS + 5 * NN, out);
        return 0;
    }

    template int separable_factors<8>(const float *, const float *, double (&)[8][8], double (&)[8][8], double (&)[8], double (&)[8]);
    template int element_lane_tables<4>(const float *, const float *, float *);
    template int element_lane_tables<5>(const float *, const float *, float *);
} // namespace cuddh_k

extern "C"
{
    int cuddh_element_lane_tables(int nb, const float *h_D, const float *h_G, float *h_out)
    {
        if (!h_D || !h_G || !h_out)
            return 1; // hipErrorInvalidValue
        if (nb == 4)
            return cuddh_k::element_lane_tables<4>(h_D, h_G, h_out);
        if (nb == 5)
            return cuddh_k::element_lane_tables<5>(h_D, h_G, h_out);
        return 1;
    }
}
