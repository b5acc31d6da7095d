// rtus_bracket.h — the bracket-and-refine core of the table kernels that minimise a travel time T over one scan coordinate
// (rtus_surface.hip: T(x) along a sampled profile, three instantiations; rtus_lens_pipe.hip: T(beta) along the pipe's circle).
// Each scans the fp32 SIGN of T' over its scan points P_j = x0 + j h, keeps the three best - -> + brackets per (element, focal
// point) in a sorted triple (RTUS_KEEP3) and refines a kept bracket in fp64: its fp64 bracket (rtus_bracket_fix), then a
// safeguarded Newton on T' = 0 (rtus_newton_min).  Device-only, no state.  WHICH kept brackets are refined and which refined
// roots count stays with each kernel: the rules differ.  A new user brings T(x) with .t, .d1, .d2.
//
// Rounding: the two files set floating-point contraction differently and read this header above their choice, so nothing here
// multiplies into an add (x + step, -d1 / d2, 0.5 * (lo + hi) and compares only); a multiply-add added here is written fma().
// Evaluations: the callers' T carries a warm start from call to call (the skip leg's u, the pipe's alpha), so the order and number
// of calls stated below are part of the result's bits.
// Not users: skip_inner, lens_leg_min's cell solve and pipe_T's alpha solve look like rtus_newton_min and differ in substance
// (open against closed interval test, no T'' > 0 test in skip_inner, other stop rules and iteration caps).
#pragma once

// insert (t, j) into the sorted triple (T[0] <= T[1] <= T[2]): selects on values (references invite a phi of pointers -> scratch)
#define RTUS_KEEP3(t, j, T, J)                                                                              \
    do {                                                                                                    \
        const bool c0_ = (t) < T[0], c1_ = (t) < T[1], c2_ = (t) < T[2];                                    \
        T[2] = c1_ ? T[1] : (c2_ ? (t) : T[2]);  J[2] = c1_ ? J[1] : (c2_ ? (j) : J[2]);                    \
        T[1] = c0_ ? T[0] : (c1_ ? (t) : T[1]);  J[1] = c0_ ? J[0] : (c1_ ? (j) : J[1]);                    \
        T[0] = c0_ ? (t) : T[0];                 J[0] = c0_ ? (j) : J[0];                                   \
    } while (0)

// The fp32 scan saw T' < 0 at P_j and > 0 at P_j+1 (of m scan points); d1_at(jp) is T' at P_jp in fp64.  Where an fp32 sign was
// wrong (|T'| below fp32 resolution) the fp64 signs pick the neighbouring cell: true with T'(P_jl) < 0 < T'(P_jh), (jl, jh) one of
// (j - 1, j), (j, j + 1), (j + 1, j + 2).  Calls d1_at(j), d1_at(j + 1), then at most one of d1_at(j - 1), d1_at(j + 2).
template <class D1>
__device__ __forceinline__ bool rtus_bracket_fix(int j, int m, D1 d1_at, int& jl, int& jh)
{
    jl = j;
    jh = j + 1;
    const double dlo = d1_at(j);
    const double dhi = d1_at(j + 1);
    if (!(dlo < 0.0)) {                                      // the root is left of P_j
        if (!(dhi > 0.0) || j == 0) return false;
        jh = j;
        jl = j - 1;
        return d1_at(jl) < 0.0;
    }
    if (!(dhi > 0.0)) {                                      // ... or right of P_j+1
        if (j + 2 >= m) return false;
        jl = j + 1;
        jh = j + 2;
        return d1_at(jh) > 0.0;
    }
    return true;
}

// Safeguarded Newton on T'(x) = 0 inside [lo, hi], T'(lo) < 0 < T'(hi), from the midpoint: bisection when T'' <= 0 or a step
// leaves [lo, hi]; stops on T' == 0, on a step within tol where T'' > 0, or on a bracket within tol; at most 100 steps.  Returns
// T_at's result at the last iterate, which is left in x.  Calls T_at once per iterate.
template <class TF>
__device__ __forceinline__ auto rtus_newton_min(TF T_at, double lo, double hi, double tol, double& x)
{
    x = 0.5 * (lo + hi);
    auto v = T_at(x);
    for (int it = 0; it < 100; ++it) {
        if (v.d1 == 0.0) break;
        if (v.d1 < 0.0) lo = x; else hi = x;
        const double step = -v.d1 / v.d2;
        // converged: the last Newton step is taken even when it rounds onto x (a bisection there would jump away from the root)
        const bool done = (v.d2 > 0.0 && fabs(step) <= tol) || !(hi - lo > tol);
        double xn = x + step;
        if (!(v.d2 > 0.0) || !(xn >= lo && xn <= hi)) xn = done ? x : 0.5 * (lo + hi);
        x = xn;
        v = T_at(x);
        if (done) break;
    }
    return v;
}
