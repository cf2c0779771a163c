// Which kernel a DDH plan runs: see kernels/ddh_resolve.hpp.  Plain C++: nothing here touches the device.
#include "ddh_resolve.hpp"

#include "cuddh_hip.h"

namespace cuddh_k
{
    namespace
    {
        constexpr int REFUSED = 1; // hipErrorInvalidValue

        // kernel 5 plans with fewer subdomains than this stay on the matrix form under auto: the element-lane form puts four
        // subdomains into a wavefront, so a small plan leaves SIMDs empty that the matrix form would use.  Measured on one MI355X
        // (profiles/r08/ddh_rates_by_form.txt, three rounds per size): 1,024 subdomains 8.8 / 20.4 ms per action (matrix /
        // element-lane), 4,096 19.7 / 20.5, 8,192 73.8 / 71.6, 16,384 70.6 / 68.1, 65,536 273.6 / 260.4.  8,192 is the smallest
        // measured size at which the element-lane form won every round, not a crossover: nothing was measured between 4,096 and
        // 8,192, and the 8,192 case is another problem (256 x 512 rectangular elements, nt 10,240).  The form belongs to the plan,
        // so a small launch of a large plan (a few subdomains, the rim launch of a multi-GPU schedule) runs four subdomains per
        // wavefront as well, at a size where this form measured slower on its own.
        constexpr int ELEMENT_LANE_MIN_DOMAINS = 8192;
        // what auto takes as the assembly of head 2 from that size on: the form over the LDS pipe, the same bits as the DPP form.
        // One MI355X, 65,536 subdomains, three rounds each (profiles/r33/bench_ab.txt): 137.79 to 138.05 ms per step with DPP,
        // 133.92 to 134.20 fetched.  Smaller plans, where head 2 is in effect only when it is forced, keep DPP: not measured
        constexpr int DDH_ASSEMBLY_AUTO = 2;
        // kernel 12 against kernel 1 under auto (n_basis 5, block 4), the same rule: the smallest measured subdomain count at which
        // kernel 12 won every round by more than the rounds differ.  One MI355X, ms per action, kernel 1 / kernel 12, three rounds
        // each (profiles/r19/ddh_nb5_rates.txt): 64 subdomains 8.51 / 8.31 (1.02 x, rounds within 0.7 %), 256 8.58 / 8.28, 1,024
        // 18.7 / 8.33 (2.2 x), 4,096 66.9 / 8.83 (7.6 x), 16,384 253.4 / 29.3 (8.6 x).  Nothing was measured below 64: there auto
        // keeps kernel 1.  Up to 4,096 subdomains a launch of kernel 12 is one round of wavefronts and costs what one wavefront
        // costs.
        constexpr int ELEMENT_LANE5_MIN_DOMAINS = 64;

        constexpr unsigned S = DDH_STRUCTURE, U = DDH_UNIFORM, I = DDH_INTERIOR;
        constexpr unsigned seq(unsigned a, unsigned b = 0, unsigned c = 0, unsigned d = 0, unsigned e = 0)
        {
            return a | (b << 4) | (c << 8) | (d << 12) | (e << 16);
        }

        // What a kernel is tied to and which forms it has.  The one table of kernel numbers: the shapes and precisions of
        // cuddh_hip_ddh_plan_create, the checks (in the order plan creation runs them; the kernel needs them all, kernel 5 all
        // but the element-lane tables, without which it keeps the matrix form), and
        //   grids: takes per-subdomain time grids.  The kernels that hold ONE subdomain per wavefront or workgroup do; 6 and 7
        //       hold two per wavefront and 12 four, on one grid; 13 holds four and marches once per grid among them;
        //   rk4: has an RK4 form.  RK4 keeps two registers more per value than RK2 (wh_march); a form is built only where it
        //       compiles without scratch and at the occupancy of its RK2 form ("Runge-Kutta 4", the table from the
        //       code objects): kernel 11 and kernel 5's element-lane form, sixteen values per lane, spill 216 to 236 bytes in the
        //       form without x, and kernels 3 and 4 go from 86 / 90 to 98 / 99 vector registers, five wavefronts per SIMD to
        //       four.  Kernels 6 and 7 have none by decision, and kernel 12 (25 values per lane, one wavefront per SIMD already
        //       in RK2) has none either; kernel 13 is the same two kernels.  The label-built plans' kernels 9 (wh_march around
        //       its LDS assembly, no scratch) and 10 (kernel 1's form with the plan's lists) have one;
        //   owner_rule: cuddh_hip_ddh_plan_set_owner_rule applies.
        struct KernelTraits
        {
            int nb, nel1d;  // the shape, 0: any
            int real_bytes; // 4: fp32 only, 8: fp64 only, 0: both
            unsigned checks;
            bool grids, rk4, owner_rule;
        };
        constexpr KernelTraits KERNELS[14] = {
            {},
            /*  1 */ {0, 0, 0, 0, true, true, false},
            /*  2 */ {4, 4, 0, seq(S), true, true, false},
            /*  3 */ {4, 4, 0, seq(S), true, false, false},
            /*  4 */ {4, 4, 0, seq(S), true, false, false},
            /*  5 */ {4, 4, 4, seq(S, U, I, DDH_DENSE, DDH_LANE), true, true, false}, // time grids and RK4: in the matrix form
            /*  6 */ {8, 2, 0, seq(S), false, false, false},
            /*  7 */ {8, 2, 4, seq(S, U, DDH_SEP8), false, false, false},
            /*  8 */ {4, 4, 8, seq(S, U, I, DDH_DENSE), true, true, false},
            /*  9 */ {4, 0, 0, 0, true, true, false}, // label-built, at most 16 elements per subdomain
            /* 10 */ {0, 0, 0, 0, true, true, false}, // label-built
            /* 11 */ {4, 8, 4, seq(S, I, U, DDH_LANE), true, false, true},
            /* 12 */ {5, 4, 4, seq(S, I, U, DDH_LANE), false, false, true},
            /* 13 */ {0, 4, 4, seq(S, I, U, DDH_LANE), true, false, true}, // n_basis 4 (there: S, U, I) or 5
        };
        // what auto takes, the first that fits the shape and whose checks held; kernel 1 (label-built: 10) otherwise.  2, 4, 8 and
        // 13 on request only
        constexpr int AUTO_PREFERENCE[] = {5, 3, 7, 6, 11, 12, 9};

        bool general(const DdhShape &s) { return s.mx_elems > 0; }

        bool shape_valid(const DdhShape &s)
        {
            if (s.nb < 2 || s.nb > 10)
                return false;
            if (general(s))
                return s.mx_elems <= 256 && s.nb * s.nb * s.mx_elems <= DDH_GENERAL_MAX_NODES;
            return s.nel1d >= 1 && s.nel1d <= 16 && s.nb * s.nb * s.nel1d * s.nel1d <= DDH_BLOCK_MAX_NODES;
        }

        // is kernel k built for this shape and precision?
        bool fits(const DdhShape &s, int k)
        {
            const KernelTraits &t = KERNELS[k];
            if (general(s) != (k == 9 || k == 10))
                return false;
            if (t.real_bytes != 0 && t.real_bytes != (s.is_f64 ? 8 : 4))
                return false;
            if (k == 9)
                return s.nb == 4 && s.mx_elems <= 16;
            if (k == 13)
                return (s.nb == 4 || s.nb == 5) && s.nel1d == 4;
            return (t.nb == 0 || t.nb == s.nb) && (t.nel1d == 0 || t.nel1d == s.nel1d);
        }

        unsigned checks_of(const DdhShape &s, int k) { return k == 13 && s.nb == 4 ? seq(S, U, I, DDH_LANE) : KERNELS[k].checks; }

        bool checks_held(const DdhShape &s, int k, unsigned facts)
        {
            for (unsigned c = checks_of(s, k); c != 0; c >>= 4)
                if (!(facts & ddh_fact(c & 15)) && !(k == 5 && (c & 15) == DDH_LANE))
                    return false;
            return true;
        }

        // auto's candidates on this shape, in order of preference; 0 ends the list
        int auto_candidate(const DdhShape &s, int i)
        {
            for (const int k : AUTO_PREFERENCE)
                if (fits(s, k) && !(k == 12 && s.n_domains < ELEMENT_LANE5_MIN_DOMAINS) && i-- == 0)
                    return k;
            return 0;
        }

        bool request_valid(const DdhShape &s, int request)
        {
            if (!shape_valid(s) || request < 0 || request > 13)
                return false;
            if (request == 0)
                return true;
            return fits(s, request);
        }
    } // namespace

    int ddh_checks(const DdhShape &s, int request)
    {
        if (!request_valid(s, request))
            return -1;
        if (general(s))
            return 0;
        // auto's first candidate needs what its later ones need and more (5 over 3, 7 over 6)
        const int k = request != 0 ? request : auto_candidate(s, 0);
        return k ? static_cast<int>(checks_of(s, k)) : 0;
    }

    int ddh_resolve(const DdhShape &s, int request, unsigned facts, int current, const DdhOptions &o, int setting, DdhResolved &out)
    {
        if (!request_valid(s, request) || current < 0 || current > 13 || o.sweep_form < 0 || o.sweep_form > 3 || o.chain_order < 0 || o.chain_order > 2)
            return REFUSED;
        int k = current;
        if (k == 0) // plan creation: the request where its checks held, or auto's first candidate whose checks held
        {
            if (request != 0 && !checks_held(s, request, facts))
                return REFUSED;
            k = request;
            for (int i = 0; k == 0; ++i)
            {
                const int c = auto_candidate(s, i);
                k = c == 0 ? (general(s) ? 10 : 1) : (checks_held(s, c, facts) ? c : 0);
            }
        }
        else if (!fits(s, k))
            return REFUSED;
        // an option the kernel has no form for: a request is refused, an auto choice moves
        if (o.time_grids && !KERNELS[k].grids)
        {
            if (request != 0)
                return REFUSED;
            k = 1;
        }
        if (o.rk4 && !KERNELS[k].rk4)
        {
            if (request != 0)
                return REFUSED;
            k = k == 3 ? 2 : 1; // 2: kernel 3's lane map without the folded DPP reads
        }
        // kernel 5's element-lane form holds four subdomains per wavefront on one time grid and has no RK4 form
        const bool lane_form = k == 5 && (facts & ddh_fact(DDH_LANE)) && !o.time_grids && !o.rk4;
        if (o.sweep_form >= 2 && !lane_form)
            return REFUSED;
        if (setting == DDH_SET_CHAIN_ORDER && o.chain_order == 2 && !lane_form)
            return REFUSED;
        if (setting == DDH_SET_OWNER_RULE && !KERNELS[k].owner_rule)
            return REFUSED;
        out.kernel = k;
        // the form and the order are properties of the plan alone, never of a launch: differently partitioned launches of one
        // plan are compared bitwise.  Auto gives the paired chains exactly where auto gave the form: a form forced with
        // set_sweep_form(2 | 3) is what fixtures and diagnostics ask for, and its bits stay.
        out.form = k != 5 ? 0 : !lane_form ? 1 : o.sweep_form != 0 ? o.sweep_form : s.n_domains >= ELEMENT_LANE_MIN_DOMAINS ? 2 : 1;
        out.order = out.form < 2 ? 0 : o.chain_order != 0 ? o.chain_order : o.sweep_form == 0 ? 2 : 1;
        return 0;
    }

    int ddh_forcing(const DdhResolved &r, int sweep_form, int chain_order, int forcing)
    {
        if (r.order != 2)
            return 0;
        if (forcing == 2)
            return 2;
        return forcing == 0 && sweep_form == 0 && chain_order == 0 ? 2 : 1;
    }

    int ddh_forcing_accepted(const DdhShape &s, int request, unsigned facts, int current, const DdhOptions &o, int forcing)
    {
        if (forcing < 0 || forcing > 2)
            return REFUSED;
        if (forcing != 2)
            return 0;
        DdhResolved unused;
        return ddh_resolve(s, request, facts, current, DdhOptions{o.time_grids, o.rk4, o.sweep_form, 2}, DDH_SET_CHAIN_ORDER, unused);
    }

    int ddh_march(int forcing_now, int sweep_form, int chain_order, int forcing, int march)
    {
        if (forcing_now != 2)
            return 0;
        if (march == 2)
            return 2;
        return march == 0 && sweep_form == 0 && chain_order == 0 && forcing == 0 ? 2 : 1;
    }

    int ddh_march_accepted(const DdhShape &s, int request, unsigned facts, int current, const DdhOptions &o, int march)
    {
        if (march < 0 || march > 2)
            return REFUSED;
        return march != 2 ? 0 : ddh_forcing_accepted(s, request, facts, current, o, 2);
    }

    int ddh_head(int march_now, int head)
    {
        if (march_now != 2)
            return 0;
        return head == 1 ? 1 : 2;
    }

    int ddh_head_accepted(const DdhShape &s, int request, unsigned facts, int current, const DdhOptions &o, int head)
    {
        if (head < 0 || head > 2)
            return REFUSED;
        return head != 2 ? 0 : ddh_march_accepted(s, request, facts, current, o, 2);
    }

    int ddh_assembly(int head_now, int n_domains, int assembly)
    {
        if (head_now != 2)
            return 0;
        if (assembly != 0)
            return assembly == 2 ? 2 : 1;
        return n_domains >= ELEMENT_LANE_MIN_DOMAINS ? DDH_ASSEMBLY_AUTO : 1;
    }

    int ddh_assembly_accepted(int head_now, int assembly)
    {
        if (assembly < 0 || assembly > 2)
            return REFUSED;
        return assembly == 2 && head_now != 2 ? REFUSED : 0;
    }
} // namespace cuddh_k

extern "C"
{
    int cuddh_ddh_resolve(int nb, int nel1d, int n_domains, int is_f64, int mx_elems, int request, int facts, int current, int time_grids, int rk4,
                          int sweep_form, int chain_order, int setting, int *out)
    {
        using namespace cuddh_k;
        if (!out)
            return 1; // hipErrorInvalidValue
        const DdhShape s{nb, nel1d, n_domains, is_f64 ? 1 : 0, mx_elems};
        out[3] = ddh_checks(s, request);
        DdhResolved r{0, 0, 0};
        const int err = ddh_resolve(s, request, static_cast<unsigned>(facts), current, DdhOptions{time_grids, rk4, sweep_form, chain_order}, setting, r);
        out[0] = r.kernel;
        out[1] = r.form;
        out[2] = r.order;
        return err;
    }

    int cuddh_ddh_resolve_forcing(int nb, int nel1d, int n_domains, int is_f64, int mx_elems, int request, int facts, int current, int time_grids, int rk4,
                                  int sweep_form, int chain_order, int forcing, int setting, int *out)
    {
        using namespace cuddh_k;
        if (!out)
            return 1; // hipErrorInvalidValue
        const DdhShape s{nb, nel1d, n_domains, is_f64 ? 1 : 0, mx_elems};
        const DdhOptions o{time_grids, rk4, sweep_form, chain_order};
        DdhResolved r{0, 0, 0};
        int err = ddh_resolve(s, request, static_cast<unsigned>(facts), current, o, setting, r);
        if (!err && (forcing < 0 || forcing > 2 || (setting == DDH_SET_FORCING && ddh_forcing_accepted(s, request, static_cast<unsigned>(facts), current, o, forcing))))
            err = 1;
        out[0] = err ? 0 : r.kernel;
        out[1] = err ? 0 : r.form;
        out[2] = err ? 0 : r.order;
        out[3] = err ? 0 : ddh_forcing(r, sweep_form, chain_order, forcing);
        return err;
    }

    int cuddh_ddh_resolve_march(int nb, int nel1d, int n_domains, int is_f64, int mx_elems, int request, int facts, int current, int time_grids, int rk4,
                                int sweep_form, int chain_order, int forcing, int march, int setting, int *out)
    {
        using namespace cuddh_k;
        if (!out)
            return 1; // hipErrorInvalidValue
        const DdhShape s{nb, nel1d, n_domains, is_f64 ? 1 : 0, mx_elems};
        const DdhOptions o{time_grids, rk4, sweep_form, chain_order};
        int err = cuddh_ddh_resolve_forcing(nb, nel1d, n_domains, is_f64, mx_elems, request, facts, current, time_grids, rk4, sweep_form, chain_order, forcing,
                                            setting == DDH_SET_MARCH ? DDH_SET_NONE : setting, out);
        if (!err && (march < 0 || march > 2 || (setting == DDH_SET_MARCH && ddh_march_accepted(s, request, static_cast<unsigned>(facts), current, o, march))))
            err = 1;
        if (err)
            out[0] = out[1] = out[2] = out[3] = 0;
        out[4] = err ? 0 : ddh_march(out[3], sweep_form, chain_order, forcing, march);
        return err;
    }

    int cuddh_ddh_resolve_head(int nb, int nel1d, int n_domains, int is_f64, int mx_elems, int request, int facts, int current, int time_grids, int rk4,
                               int sweep_form, int chain_order, int forcing, int march, int head, int setting, int *out)
    {
        using namespace cuddh_k;
        if (!out)
            return 1; // hipErrorInvalidValue
        const DdhShape s{nb, nel1d, n_domains, is_f64 ? 1 : 0, mx_elems};
        const DdhOptions o{time_grids, rk4, sweep_form, chain_order};
        int err = cuddh_ddh_resolve_march(nb, nel1d, n_domains, is_f64, mx_elems, request, facts, current, time_grids, rk4, sweep_form, chain_order, forcing,
                                          march, setting == DDH_SET_HEAD ? DDH_SET_NONE : setting, out);
        if (!err && (head < 0 || head > 2 || (setting == DDH_SET_HEAD && ddh_head_accepted(s, request, static_cast<unsigned>(facts), current, o, head))))
            err = 1;
        if (err)
            out[0] = out[1] = out[2] = out[3] = out[4] = 0;
        out[5] = err ? 0 : ddh_head(out[4], head);
        return err;
    }

    int cuddh_ddh_resolve_assembly(int nb, int nel1d, int n_domains, int is_f64, int mx_elems, int request, int facts, int current, int time_grids, int rk4,
                                   int sweep_form, int chain_order, int forcing, int march, int head, int assembly, int setting, int *out)
    {
        using namespace cuddh_k;
        if (!out)
            return 1; // hipErrorInvalidValue
        int err = cuddh_ddh_resolve_head(nb, nel1d, n_domains, is_f64, mx_elems, request, facts, current, time_grids, rk4, sweep_form, chain_order, forcing,
                                         march, head, setting == DDH_SET_ASSEMBLY ? DDH_SET_NONE : setting, out);
        if (!err && (assembly < 0 || assembly > 2 || (setting == DDH_SET_ASSEMBLY && ddh_assembly_accepted(out[5], assembly))))
            err = 1;
        if (err)
            out[0] = out[1] = out[2] = out[3] = out[4] = out[5] = 0;
        out[6] = err ? 0 : ddh_assembly(out[5], n_domains, assembly);
        return err;
    }
}
