// rtus_lens.h — the curved lens's arithmetic shared by the kernels that solve a leg through it (rtus_lens_fermat.hip: element to
// a point in the water; rtus_lens_pipe.hip: element to a point of the pipe's outer surface) or walk one (rtus_amp_pipe.hip).  Interface P(alpha) = h(alpha)
// (sin alpha, cos alpha) with the aplanatic h(alpha) of main_rt.py:180-189 and its derivatives main_rt.py:192-214.
#pragma once
#include "rtus_device.h"

template <typename R> __device__ __forceinline__ R rsqrt_r(R v);
template <> __device__ __forceinline__ float rsqrt_r<float>(float v) { return __builtin_amdgcn_rsqf(v); }
template <> __device__ __forceinline__ double rsqrt_r<double>(double v)
{
    double y = (double)__builtin_amdgcn_rsqf((float)v);
    const double e = fma(-v * y, y, 1.0);
    y = fma(y * e, fma(e, 0.375, 0.5), y);                 // cubic step: 1e-7 -> ~1e-21 (rounding-limited)
    return y;
}
// 1/v to ~1e-7 through the fp32 pipe: Newton steps, the T polish and the alpha output only multiply small
// corrections by it (IEEE fp64 divide costs 25 ns per wave-op, this ~7 ns)
template <typename R> __device__ __forceinline__ R rcp_r(R v) { return (R)__builtin_amdgcn_rcpf((float)v); }

// sin and cos for |a| <= 1 rad (the lens is only defined inside +-50.6 deg, main_rt.py:479): Taylor polynomials
// in Horner form, truncation 4e-23 (fp64, degree 21/22) / 2.5e-8 (fp32, degree 9/10) — the generic sincos spends
// most of its time on a range reduction that is never needed here.
template <typename R> __device__ __forceinline__ void sincos_poly(R a, R& s, R& c);
template <> __device__ __forceinline__ void sincos_poly<float>(float a, float& s, float& c)
{
    // degree 9 / 10: the first dropped terms, a^11/11! and a^12/12!, are 2.5e-8 and 2.1e-9 at |a| = 1 — below half an fp32 ulp of
    // sin 1 and cos 1 (and 6e-9 / 5e-10 at the lens's own +-0.884 rad)
    const float x2 = a * a;
    float ps = fmaf(x2, 2.7557319e-6f, -1.9841270e-4f);     //  1/9!, -1/7!
    ps = fmaf(x2, ps, 8.3333333e-3f);                        //  1/5!
    ps = fmaf(x2, ps, -1.6666667e-1f);                       // -1/3!
    s = fmaf(a * x2, ps, a);
    float pc = fmaf(x2, -2.7557319e-7f, 2.4801587e-5f);     // -1/10!, 1/8!
    pc = fmaf(x2, pc, -1.3888889e-3f);                       // -1/6!
    pc = fmaf(x2, pc, 4.1666667e-2f);                        //  1/4!
    pc = fmaf(x2, pc, -0.5f);
    c = fmaf(x2, pc, 1.0f);
}
template <> __device__ __forceinline__ void sincos_poly<double>(double a, double& s, double& c)
{
    const double x2 = a * a;
    double ps = fma(x2, -1.9572941063391263e-20, 8.2206352466243295e-18);   // -1/21!, 1/19!
    ps = fma(x2, ps, -2.8114572543455206e-15);               // -1/17!
    ps = fma(x2, ps, 7.6471637318198164e-13);                //  1/15!
    ps = fma(x2, ps, -1.6059043836821613e-10);               // -1/13!
    ps = fma(x2, ps, 2.5052108385441720e-8);                 //  1/11!
    ps = fma(x2, ps, -2.7557319223985893e-6);                // -1/9!
    ps = fma(x2, ps, 1.9841269841269841e-4);                 //  1/7!
    ps = fma(x2, ps, -8.3333333333333333e-3);                // -1/5!
    ps = fma(x2, ps, 1.6666666666666666e-1);                 //  1/3!
    s = fma(-(a * x2), ps, a);
    double pc = fma(x2, 8.8967913924505741e-22, -4.1103176233121648e-19);   // 1/22!, -1/20!
    pc = fma(x2, pc, 1.5619206968586225e-16);                //  1/18!
    pc = fma(x2, pc, -4.7794773323873853e-14);               // -1/16!
    pc = fma(x2, pc, 1.1470745597729725e-11);                //  1/14!
    pc = fma(x2, pc, -2.0876756987868100e-9);                // -1/12!
    pc = fma(x2, pc, 2.7557319223985888e-7);                 //  1/10!
    pc = fma(x2, pc, -2.4801587301587302e-5);                // -1/8!
    pc = fma(x2, pc, 1.3888888888888889e-3);                 //  1/6!
    pc = fma(x2, pc, -4.1666666666666664e-2);                // -1/4!
    pc = fma(x2, pc, 0.5);
    c = fma(-x2, pc, 1.0);
}
template <typename R> __device__ __forceinline__ void sincos_r(R a, R* s, R* c);
template <> __device__ __forceinline__ void sincos_r<float>(float a, float* s, float* c) { sincosf(a, s, c); }
template <> __device__ __forceinline__ void sincos_r<double>(double a, double* s, double* c) { sincos(a, s, c); }

// The lens constants as the solver's arithmetic reads them.  On gfx950 an fp32 VALU instruction with an SGPR operand
// issues at half the rate of one with VGPR / inline-constant operands (4.2 vs 2.3 cycles, scripts/ubench_issue3.hip), and
// kernel arguments live in SGPRs: the fp32 instantiation keeps per-lane (VGPR) copies, made opaque to the compiler so
// that it does not fold them back into scalar operands.  (fp64 instructions cost 4.2 cycles either way: no copies.)
template <typename R> struct LensConst {
    R c1inv, c2inv, phi_3, twoTc, C4A, inv2A;
    int poly_trig;
};

// The constants of lens L for the alpha interval [a_lo, a_hi] (host): sin / cos by polynomial where the interval allows it
template <typename R> static inline LensConst<R> make_lens_const(const rtus_lens& L, double a_lo, double a_hi)
{
    const LensK kk = make_lens_k(L);
    LensConst<R> k;
    k.c1inv = (R)(1.0 / L.c1); k.c2inv = (R)(1.0 / L.c2);
    k.phi_3 = (R)kk.phi_3; k.twoTc = (R)kk.twoTc; k.C4A = (R)kk.C4A; k.inv2A = (R)(1.0 / kk.twoA);
    k.poly_trig = (a_lo >= -1.0 && a_hi <= 1.0) ? 1 : 0;
    return k;
}
// g' below this at a minimum of the lens leg's time: suspect, a second minimum may exist (rtus_tt_lens and, for its inner solve,
// rtus_tt_pipe).  The lens's own time scales the constant measured on the reference lens: 7.5e-6 s/rad^2, twice the largest g' seen at
// an interior minimum of a pair with two minima (h0 / c2 = 5.96e-5 s; scripts/study_lens_minima.py)
static inline double lens_gp_min(const rtus_lens& L) { return 0.125 * L.h0 / L.c2; }

// the lens point P, its tangent P' and (WITH_P2) P'' at alpha (lens_time's formulas)
template <bool POLY, bool WITH_P2>
__device__ __forceinline__ void lens_point(const LensConst<double>& k, double alpha, double& px, double& pz, double& p1x, double& p1z,
                                           double& p2x, double& p2z)
{
    double s, c;
    if (POLY) sincos_poly<double>(alpha, s, c);
    else sincos_r<double>(alpha, &s, &c);
    const double B = k.phi_3 * c - k.twoTc, B1 = -k.phi_3 * s, B2 = -k.phi_3 * c;
    const double disc = B * B - k.C4A;
    const double rS = rsqrt_r<double>(disc), S = disc * rS, BrS = B * rS;
    const double h = -(B + S) * k.inv2A, h1 = -B1 * (1.0 + BrS) * k.inv2A;
    px = h * s; pz = h * c;
    p1x = h1 * s + pz; p1z = h1 * c - px;
    if (WITH_P2) {
        const double h2 = -(B2 * (1.0 + BrS) + B1 * B1 * rS * (1.0 - BrS * BrS)) * k.inv2A;
        p2x = h2 * s + 2.0 * h1 * c - px; p2z = h2 * c - 2.0 * h1 * s - pz;
    }
}
template <bool POLY>
__device__ __forceinline__ void lens_point(const LensConst<double>& k, double alpha, double& px, double& pz, double& p1x, double& p1z)
{
    double p2x, p2z;
    lens_point<POLY, false>(k, alpha, px, pz, p1x, p1z, p2x, p2z);
}

// T(alpha), g = dT/dalpha and (WITH_GP) g' for one (A, F).  Without g' the second derivatives h'', P'' are skipped:
// about a quarter of the arithmetic.
template <typename R, bool WITH_GP, bool POLY>
__device__ __forceinline__ void lens_time(const LensConst<R>& k, R alpha, R xa, R za, R xf, R zf, R& T, R& g,
                                          R& gp)
{
    R s, c;
    if (POLY) sincos_poly<R>(alpha, s, c);                  // [a_lo, a_hi] inside +-1 rad: chosen at launch
    else sincos_r<R>(alpha, &s, &c);
    const R B = k.phi_3 * c - k.twoTc;                      // main_rt.py:184
    const R B1 = -k.phi_3 * s, B2 = -k.phi_3 * c;           // B', B''
    const R disc = B * B - k.C4A;
    const R rS = rsqrt_r<R>(disc);                          // 1/S
    const R S = disc * rS;
    const R h = -(B + S) * k.inv2A;                         // :171-177 root [1]
    const R BrS = B * rS;
    const R h1 = -B1 * (R(1) + BrS) * k.inv2A;              // :199-212
    const R px = h * s, pz = h * c;                         // :220-221
    const R p1x = h1 * s + pz, p1z = h1 * c - px;           // :231-232
    const R ax = px - xa, az = pz - za, fx = px - xf, fz = pz - zf;
    const R ra = rsqrt_r<R>(ax * ax + az * az), rf = rsqrt_r<R>(fx * fx + fz * fz);
    const R la = (ax * ax + az * az) * ra, lf = (fx * fx + fz * fz) * rf;
    const R ua = (ax * p1x + az * p1z) * ra, uf = (fx * p1x + fz * p1z) * rf;     // u . P'
    T = la * k.c1inv + lf * k.c2inv;
    g = ua * k.c1inv + uf * k.c2inv;
    if (WITH_GP) {
        const R h2 = -(B2 * (R(1) + BrS) + B1 * B1 * rS * (R(1) - BrS * BrS)) * k.inv2A;
        const R p2x = h2 * s + R(2) * h1 * c - px, p2z = h2 * c - R(2) * h1 * s - pz;
        const R pp = p1x * p1x + p1z * p1z;
        gp = ((pp - ua * ua) * ra + (ax * p2x + az * p2z) * ra) * k.c1inv
           + ((pp - uf * uf) * rf + (fx * p2x + fz * p2z) * rf) * k.c2inv;
    }
}

// T(alpha) alone: no P', no g.  T is stationary in alpha at the ray (Fermat), so evaluated delta away from the minimiser it is off by
// g' delta^2 / 2 — with g' ~ 1e-4 s/rad^2: 5e-15 s at delta = 1e-5 rad (fp32's tolerance), 5e-21 s at 1e-8 rad (fp64's).
template <typename R, bool POLY>
__device__ __forceinline__ R lens_time_only(const LensConst<R>& k, R alpha, R xa, R za, R xf, R zf)
{
    R s, c;
    if (POLY) sincos_poly<R>(alpha, s, c);
    else sincos_r<R>(alpha, &s, &c);
    const R B = k.phi_3 * c - k.twoTc;                      // main_rt.py:184
    const R disc = B * B - k.C4A;
    const R S = disc * rsqrt_r<R>(disc);
    const R h = -(B + S) * k.inv2A;                         // :171-177 root [1]
    const R px = h * s, pz = h * c;                         // :220-221
    const R ax = px - xa, az = pz - za, fx = px - xf, fz = pz - zf;
    const R da = ax * ax + az * az, df = fx * fx + fz * fz;
    return da * rsqrt_r<R>(da) * k.c1inv + df * rsqrt_r<R>(df) * k.c2inv;
}
