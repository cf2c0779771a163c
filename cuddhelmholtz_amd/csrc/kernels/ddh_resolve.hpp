// Which local-solve kernel a DDH plan runs (ddh.hip), in which sweep form and chain order, or that a request is refused: the
// rule as host-only code on plain integers (src/ddh_resolve.cpp, no HIP).  ddh.hip establishes the facts on the device, calls
// ddh_resolve() at the end of plan creation and of every setter whose argument enters the rule, and stores the outcome; tests
// read the rule through cuddh_ddh_resolve (include/cuddh_hip.h) without a GPU.  DESIGN.md 4.3.
#pragma once

namespace cuddh_k
{
    // What plan creation establishes about a descriptor, one after the other.  A check or table builder runs only when every
    // one before it held, so a bit is set only with the bits of what ran before it.
    enum DdhCheck
    {
        DDH_STRUCTURE = 1, // the NB x NEL structure: elements in the order ex + NEL ey, neighbours share the expected nodes
        DDH_UNIFORM = 2,   // one metric tensor for all elements
        DDH_INTERIOR = 3,  // no trace dof lies on an element-interior node
        DDH_DENSE = 4,     // the dense element matrix was built (kernels 5 and 8)
        DDH_SEP8 = 5,      // the separable n_basis-8 tables were built (kernel 7)
        DDH_LANE = 6       // the element-lane tables were built (kernel 5's element-lane form, kernels 11, 12 and 13)
    };
    constexpr unsigned ddh_fact(int check) { return 1u << check; } // the bit of a check in `facts`

    struct DdhShape
    {
        int nb, nel1d, n_domains, is_f64;
        int mx_elems; // > 0: a label-built plan (elements per subdomain at most; nel1d is ignored)
    };

    // the options a plan holds (its setters' arguments as stored)
    struct DdhOptions
    {
        int time_grids; // != 0: per-subdomain time grids are set
        int rk4;        // != 0: the RK4 integrator
        int sweep_form, chain_order;
    };

    // the option a setter is about to store: its value must be able to take effect on the plan as it stands, while values
    // stored earlier stay where a later setter makes them idle (a chain order on a plan that takes time grids afterwards)
    enum DdhSetting
    {
        DDH_SET_NONE = 0, // plan creation, time grids, the integrator
        DDH_SET_SWEEP_FORM = 1,
        DDH_SET_CHAIN_ORDER = 2,
        DDH_SET_OWNER_RULE = 3,
        DDH_SET_FORCING = 4, // not ddh_resolve's to judge: ddh_forcing_accepted
        DDH_SET_MARCH = 5,   // nor this: ddh_march_accepted
        DDH_SET_HEAD = 6,    // nor this: ddh_head_accepted
        DDH_SET_ASSEMBLY = 7 // nor this: ddh_assembly_accepted
    };

    struct DdhResolved
    {
        int kernel; // 1 to 13
        int form;   // the sweep form in effect: 1 to 3 on kernel 5, else 0
        int order;  // the chain order in effect: 1 or 2 in the element-lane form of kernel 5, else 0
    };

    constexpr int DDH_BLOCK_MAX_NODES = 1024;  // element nodes of a subdomain: one thread each in kernel 1
    constexpr int DDH_GENERAL_MAX_NODES = 256; // the same on a label-built plan (kernels 9 and 10)

    // The checks plan creation runs for this shape and request before it can decide, in the order they run: four bits each,
    // the first in the lowest four, 0 ends the list.  -1: the request is refused on this shape whatever the descriptor holds.
    int ddh_checks(const DdhShape &shape, int request);

    // The rule.  request: the caller's kernel argument (0 auto).  facts: ddh_fact() bits of what was established.  current: the
    // kernel the plan runs now, 0 at plan creation; a later resolution starts from it and only ever moves an auto choice to a
    // kernel with the form the options need (3 to 2 and 6, 7, 11, 12 to 1 for RK4; 6, 7, 12 to 1 for time grids), so taking an
    // option back leaves the plan where it was moved.  Returns 0 and fills `out`, or 1 (hipErrorInvalidValue): refused.
    int ddh_resolve(const DdhShape &shape, int request, unsigned facts, int current, const DdhOptions &options, int setting, DdhResolved &out);

    // Where the element-lane march of kernel 5 applies the trace sources (cuddh_hip_ddh_plan_set_forcing): 1 in every WaveHoltz
    // pass, 2 in the first pass only (the later ones add what the first returned; a new rounding), 0: the plan
    // does not run the paired chains, the only ones the second schedule is built for.  `resolved`: what ddh_resolve gave for the
    // plan; the other three as stored (0 auto).  Like the paired chains, auto takes the new rounding only where everything
    // is auto: a forced form or order keeps its bits.
    int ddh_forcing(const DdhResolved &resolved, int sweep_form, int chain_order, int forcing);

    // May a plan store this forcing?  0 to 2, and 2 exactly where ddh_resolve lets the plan store chain order 2 (the arguments
    // are ddh_resolve's): accepted and idle on the matrix form of a plan that has the element-lane form, refused elsewhere.
    // Returns 0, or 1 (hipErrorInvalidValue): refused.
    int ddh_forcing_accepted(const DdhShape &shape, int request, unsigned facts, int current, const DdhOptions &options, int forcing);

    // How that march carries the velocity (cuddh_hip_ddh_plan_set_march): 1 as wh_march_pairs_once does, 2 scaled by 1 / (2 hm)
    // with its midpoint update folded into the sweep (wh_march_pairs_scaled; one more new rounding), 0: the
    // forcing in effect is not 2, the only one the scaled march is built for.  `forcing_now`: what ddh_forcing gave; the other
    // four as stored (0 auto).  Auto takes 2 only where form, order and forcing are all auto: a forced one keeps its bits.
    int ddh_march(int forcing_now, int sweep_form, int chain_order, int forcing, int march);

    // May a plan store this march?  0 to 2, and 2 exactly where it may store forcing 2.  Returns 0, or 1: refused.
    int ddh_march_accepted(const DdhShape &shape, int request, unsigned facts, int current, const DdhOptions &options, int march);

    // What the scaled march (march 2) carries as the velocity (cuddh_hip_ddh_plan_set_head): 1 q / (2 hm), multiplied by the head
    // coefficient of the first sweep's chain in every step (wh_march_pairs_scaled), 2 that product itself, so that the chain
    // opens on the state (wh_march_pairs_carried; one more new rounding), 0: the march in effect is not 2.
    // `march_now`: what ddh_march gave; `head` as stored (0 auto).  Auto is 2 wherever the march in effect is 2, forced or not:
    // only an explicit 1 keeps the bits of march 2 as they were.
    int ddh_head(int march_now, int head);

    // May a plan store this head?  0 to 2, and 2 exactly where it may store march 2.  Returns 0, or 1: refused.
    int ddh_head_accepted(const DdhShape &shape, int request, unsigned facts, int current, const DdhOptions &options, int head);

    // How the carried march (head 2) forms the neighbour sums of its sweeps (cuddh_hip_ddh_plan_set_assembly): 1 one copy of a
    // shared node forms the sum and the other takes it, DPP on the vector pipe; 2 every copy fetches the other's partial sum over
    // the LDS pipe and adds it itself (the same bits); 0: the head in effect is not 2.  `head_now`: what ddh_head
    // gave; `assembly` as stored (0 auto).  Auto is DDH_ASSEMBLY_AUTO from ELEMENT_LANE_MIN_DOMAINS subdomains on, 1 below.
    int ddh_assembly(int head_now, int n_domains, int assembly);

    // May a plan store this assembly?  0 to 2, and 2 only where the head in effect is 2.  Returns 0, or 1: refused.
    int ddh_assembly_accepted(int head_now, int assembly);
} // namespace cuddh_k
