// The host side that the per-sweep kernel files of the WaveHoltz march share (wave_lattice, wave_cells, wave_weights, wave_box and
// their _f32 counterparts): the kernels' stage arguments, the one place that fills and refuses them, the dispatch
// of run-time values (n_basis, forced, streaming) to a compile-time instantiation, and the six stage wirings behind the
// rk2_a .. rk4_4 entry points.  A family supplies its kernel, its description, its extra argument, its grid and its list of
// compile-time n_basis values as a launcher:
//   struct launch_x { <the entry points' leading arguments>; void *stream;
//                     template <typename Stage, int PSLOT> int sweep(in, F, G, out, coef) const; };
// and each of its entry points forwards to one wiring below.
#ifndef CUDDH_AMD_WAVE_SWEEP_LAUNCH_HPP
#define CUDDH_AMD_WAVE_SWEEP_LAUNCH_HPP

#include <utility>

#include "wave_stages.hpp"

namespace cuddh_k
{
    namespace wave
    {
        template <typename R>
        struct StageArgsT
        {
            const R *in[MAX_IN];
            R *out[MAX_OUT]; // may alias inputs other than a stencil input (element i is read before it is written, by the same thread)
            R coef[MAX_COEF];
        };
        using StageArgs = StageArgsT<double>;

        constexpr int invalid_value = static_cast<int>(hipErrorInvalidValue);

        // The kernel's stage arguments from the caller's, or false.  in[0]: the stencil input; F, G: both given (forced) or both
        // null (homogeneous); coef: the call's scalars, rounded to R here, once.
        template <typename Stage, typename R>
        bool stage_args(const R *const (&in)[Stage::NIN], const R *F, const R *G, R *const (&out)[Stage::NOUT], const double (&coef)[MAX_COEF],
                        StageArgsT<R> &a)
        {
            if ((F == nullptr) != (G == nullptr))
                return false;
            a = {};
            bool ok = true;
            for (int s = 0; s < Stage::NIN; ++s)
            {
                a.in[s] = in[s];
                ok = ok && in[s] && aligned16(in[s]);
            }
            if (F)
            {
                a.in[Stage::NIN] = F;
                a.in[Stage::NIN + 1] = G;
                ok = ok && aligned16(F) && aligned16(G);
            }
            for (int s = 0; s < Stage::NOUT; ++s)
            {
                a.out[s] = out[s];
                // a neighbour's thread still needs the stencil input: it is not an output
                ok = ok && out[s] && aligned16(out[s]) && out[s] != in[0];
            }
            for (int s = 0; s < MAX_COEF; ++s)
                a.coef[s] = static_cast<R>(coef[s]);
            return ok;
        }

        // a family's compile-time n_basis values; every other n_basis takes the run-time instantiation (NBT = 0)
        template <int... NBS>
        using NBasis = std::integer_sequence<int, NBS...>;

        // Run-time values become template arguments: launch(forced_c, nt_c, nbt) with std::true_type / std::false_type for
        // `forced` and for streaming non-temporally (vectors of `bytes` from NT_BYTES on), and std::integral_constant<int, NBT>
        // with NBT = nb where nb is one of NBS, else 0.
        template <int... NBS, typename Launch>
        void dispatch_sweep(int nb, NBasis<NBS...>, bool forced, long long bytes, Launch &&launch)
        {
            auto go = [&](auto nbt) { with_flags([&](auto forced_c, auto nt_c) { launch(forced_c, nt_c, nbt); }, forced, bytes >= NT_BYTES); };
            if (!((nb == NBS && (go(std::integral_constant<int, NBS>{}), true)) || ...))
                go(std::integral_constant<int, 0>{});
        }

        // The six wirings: which buffer goes into which slot of which stage (wave_stages.hpp, w = the stencil of in[0]), which
        // slot is the stencil input itself (PSLOT), and the stage's scalars.  The argument order is the entry points'.
        template <typename L, typename R>
        int rk2_a(const L &launch, double half_dt, double c, double s, const R *p, const R *q, const R *invm, const R *Hi, const R *F, const R *G,
                  R *qh, R *ph)
        {
            return launch.template sweep<Rk2AT<R>, 1>({p, p, q, invm, Hi}, F, G, {qh, ph}, {half_dt, c, s, 0.0});
        }
        template <typename L, typename R>
        int rk2_b(const L &launch, double dt, double c, double s, double filt, const R *ph, const R *qh, const R *invm, const R *Hi, const R *F,
                  const R *G, R *p, R *q, R *u, R *v)
        {
            return launch.template sweep<Rk2BT<R>, 0>({ph, qh, p, q, u, v, invm, Hi}, F, G, {p, q, u, v}, {dt, c, s, filt});
        }
        template <typename L, typename R>
        int rk4_1(const L &launch, double half_dt, double c, double s, const R *p, const R *q, const R *invm, const R *Hi, const R *F, const R *G,
                  R *ps, R *qs, R *aq, R *ap)
        {
            return launch.template sweep<Rk4FirstT<R>, 1>({p, p, q, invm, Hi}, F, G, {ps, qs, aq, ap}, {half_dt, c, s, 0.0});
        }
        template <typename L, typename R>
        int rk4_2(const L &launch, double half_dt, double c, double s, const R *ps_in, const R *p, const R *q, const R *invm, const R *Hi,
                  const R *F, const R *G, R *ps_out, R *qs, R *aq, R *ap)
        {
            return launch.template sweep<Rk4MidT<R>, 0>({ps_in, p, q, qs, aq, ap, invm, Hi}, F, G, {ps_out, qs, aq, ap}, {half_dt, c, s, 0.0});
        }
        // (rk4_2 with dt for dt/2)
        template <typename L, typename R>
        int rk4_3(const L &launch, double dt, double c, double s, const R *ps_in, const R *p, const R *q, const R *invm, const R *Hi, const R *F,
                  const R *G, R *ps_out, R *qs, R *aq, R *ap)
        {
            return rk4_2(launch, dt, c, s, ps_in, p, q, invm, Hi, F, G, ps_out, qs, aq, ap);
        }
        template <typename L, typename R>
        int rk4_4(const L &launch, double sixth_dt, double c, double s, double filt, const R *ps, const R *qs, const R *aq, const R *ap,
                  const R *invm, const R *Hi, const R *F, const R *G, R *p, R *q, R *u, R *v)
        {
            return launch.template sweep<Rk4LastT<R>, 0>({ps, p, q, qs, aq, ap, u, v, invm, Hi}, F, G, {p, q, u, v}, {sixth_dt, c, s, filt});
        }
    } // namespace wave
} // namespace cuddh_k

#endif
