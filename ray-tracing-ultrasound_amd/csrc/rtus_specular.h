// rtus_specular.h — the reduction step of rtus_specular's definition (include/rtus.h), shared by the kernels that apply it
// (rtus_specular.hip: two tables; rtus_skip_reflector.hip: one table and a closed-form up leg) so that they cannot drift apart:
// which sums count as finite, the running state of a (row, lane) over the reflector's points, and the parabola about j*.
#pragma once
#include "rtus_device.h"

// a sum that is not finite becomes NaN: every comparison with it is then false (an infinity has a zero low word, so the high word
// alone turns it into a quiet NaN)
__device__ __forceinline__ double spec_finite_or_nan(double s)
{
    const bool inf = __builtin_amdgcn_class(s, 0x204);       // -inf | +inf: one v_cmp_class_f64
    return __hiloint2double(inf ? 0x7ff80000 : __double2hiint(s), __double2loint(s));
}

struct SpecRow {
    double best, prev;
    int jbest, n_min;
    bool prev_down;
};

__device__ __forceinline__ void spec_row_init(SpecRow& w)
{
    w.best = __builtin_inf(); w.prev = __builtin_nan("");
    w.jbest = -1; w.n_min = 0; w.prev_down = false;
}

// point j's sum s (through spec_finite_or_nan) enters the row's state.  COUNT = false leaves n_min's bookkeeping out; best and jbest
// do not depend on it.
template <bool COUNT>
__device__ __forceinline__ void spec_row_step(SpecRow& w, double s, int j)
{
    if (COUNT) {
        const bool down = s < w.prev, up = w.prev < s;
        w.n_min += (w.prev_down && up) ? 1 : 0;              // the point before this one is a strict interior minimum
        w.prev_down = down;
        w.prev = s;
    }
    if (s < w.best) { w.best = s; w.jbest = j; }             // strict: the first index of the least sum
}

// the three sums about j* = js (an interior index) -> the time and the position; both stay as they are when a neighbour is not
// finite (the caller has set t = NaN, p = js)
__device__ __forceinline__ void spec_refine(double sa, double sb, double sc, int js, double& t, double& p)
{
    if (fabs(sa) <= 1.7976931348623157e308 && fabs(sc) <= 1.7976931348623157e308) {
#pragma clang fp contract(off)                               // the header's order, every operation rounded on its own
        const double d1 = sa - sc;
        const double d2 = (sa - sb) + (sc - sb);
        const double delta = 0.5 * d1 / d2;
        t = sb - (0.25 * d1) * delta;
        p = (double)js + delta;
    }
}
