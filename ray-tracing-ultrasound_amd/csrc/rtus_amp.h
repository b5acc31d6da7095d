// rtus_amp.h — the arithmetic shared by the ray amplitude kernels (rtus_amp.hip: through a measured surface; rtus_amp_pipe.hip: through
// the lens into the pipe wall): complex helpers, the plane-wave table of one wave, the three displacement coefficients by Cramer's rule
// on the boundary conditions, one interface of the ray tube, and the walk of a whole leg along its path in either direction (AmpPath,
// amp_walk: the one place where the up leg is the down leg reversed).  Definitions: include/rtus.h; oracle: tests/amplitude_numpy.py.
#pragma once
#include "rtus_device.h"

#pragma clang fp contract(off)

// The media of one fluid-solid pair reach the coefficient functions as any struct M with the members c1, r1 (the fluid's speed and
// density) and cl > ct, r2 (the solid's; amp_free reads the solid alone): AmpMedia, or a kernel's own argument block that has them.
struct AmpMedia { double c1, r1, cl, ct, r2; };

struct cd { double re, im; };
__device__ __forceinline__ cd cmk(double r, double i = 0.0) { cd c; c.re = r; c.im = i; return c; }
__device__ __forceinline__ cd cadd(cd a, cd b) { return cmk(a.re + b.re, a.im + b.im); }
__device__ __forceinline__ cd csub(cd a, cd b) { return cmk(a.re - b.re, a.im - b.im); }
__device__ __forceinline__ cd cneg(cd a) { return cmk(-a.re, -a.im); }
__device__ __forceinline__ cd cscl(cd a, double s) { return cmk(a.re * s, a.im * s); }
__device__ __forceinline__ cd cmul(cd a, cd b) { return cmk(a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re); }
__device__ __forceinline__ cd cdiv(cd a, cd b)
{
    const double d = b.re * b.re + b.im * b.im;
    return cmk((a.re * b.re + a.im * b.im) / d, (a.im * b.re - a.re * b.im) / d);
}

// vertical slowness: real >= 0 while the wave propagates, +i |.| past its critical angle (decaying in e^{i(k.x - wt)})
__device__ __forceinline__ cd amp_q(double p, double c)
{
    const double a = 1.0 / (c * c) - p * p;
    return a >= 0.0 ? cmk(sqrt(a)) : cmk(0.0, sqrt(-a));
}

// (u_n, sigma_nn / (i w), sigma_tn / (i w)) of one wave of unit amplitude: tests/amplitude_numpy.py's table (ct = 0: the fluid)
struct Wave { cd u, nn, tn; };
__device__ __forceinline__ Wave amp_wave(bool L, double p, double c, double ct, double rho, double s)
{
    const cd q = amp_q(p, c);
    const double b = 1.0 - 2.0 * ct * ct * p * p;
    const double k = 2.0 * rho * ct * ct * c * s * p;
    Wave w;
    if (L) { w.u = cscl(q, c * s); w.nn = cmk(rho * c * b); w.tn = cscl(q, k); }
    else   { w.u = cmk(c * p);     w.nn = cscl(q, k);       w.tn = cmk(-rho * c * b); }
    return w;
}

__device__ __forceinline__ cd det3(const cd m[3][3])
{
    const cd a = cmul(m[0][0], csub(cmul(m[1][1], m[2][2]), cmul(m[1][2], m[2][1])));
    const cd b = cmul(m[0][1], csub(cmul(m[1][0], m[2][2]), cmul(m[1][2], m[2][0])));
    const cd c = cmul(m[0][2], csub(cmul(m[1][0], m[2][1]), cmul(m[1][1], m[2][0])));
    return cadd(csub(a, b), c);
}

// component k of the solution of sum_j x_j col_j = rhs (Cramer)
__device__ __forceinline__ cd cramer3(const Wave cols[3], const Wave& rhs, int k)
{
    cd m[3][3], mk[3][3];
    for (int j = 0; j < 3; ++j) {
        m[0][j] = cols[j].u; m[1][j] = cols[j].nn; m[2][j] = cols[j].tn;
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) mk[i][j] = m[i][j];
    mk[0][k] = rhs.u; mk[1][k] = rhs.nn; mk[2][k] = rhs.tn;
    return cdiv(det3(mk), det3(m));
}

// fluid -> solid, transmitted into mode L (or T): incident along +n
template <class M> __device__ cd amp_fluid_solid(bool L, double p, const M& a)
{
    const Wave inc = amp_wave(true, p, a.c1, 0.0, a.r1, 1.0), ref = amp_wave(true, p, a.c1, 0.0, a.r1, -1.0);
    Wave cols[3];
    cols[0].u = cneg(ref.u); cols[0].nn = cneg(ref.nn); cols[0].tn = cmk(0.0);
    cols[1] = amp_wave(true, p, a.cl, a.ct, a.r2, 1.0);
    cols[2] = amp_wave(false, p, a.ct, a.ct, a.r2, 1.0);
    Wave rhs = inc;
    rhs.tn = cmk(0.0);
    return cramer3(cols, rhs, L ? 1 : 2);
}

// solid -> fluid from mode L (or T): incident along -n, transmitted into the couplant
template <class M> __device__ cd amp_solid_fluid(bool L, double p, const M& a)
{
    const Wave inc = amp_wave(L, p, L ? a.cl : a.ct, a.ct, a.r2, -1.0);
    const Wave tf = amp_wave(true, p, a.c1, 0.0, a.r1, -1.0);
    Wave cols[3];
    cols[0] = amp_wave(true, p, a.cl, a.ct, a.r2, 1.0);
    cols[1] = amp_wave(false, p, a.ct, a.ct, a.r2, 1.0);
    cols[2].u = cneg(tf.u); cols[2].nn = cneg(tf.nn); cols[2].tn = cmk(0.0);
    Wave rhs;
    rhs.u = cneg(inc.u); rhs.nn = cneg(inc.nn); rhs.tn = cneg(inc.tn);
    return cramer3(cols, rhs, 2);
}

// free surface: incident mode Li along +n (out of the solid), reflected into mode Lo
template <class M> __device__ cd amp_free(bool Li, bool Lo, double p, const M& a)
{
    const Wave inc = amp_wave(Li, p, Li ? a.cl : a.ct, a.ct, a.r2, 1.0);
    const Wave wl = amp_wave(true, p, a.cl, a.ct, a.r2, -1.0), wt = amp_wave(false, p, a.ct, a.ct, a.r2, -1.0);
    const cd d = csub(cmul(wl.nn, wt.tn), cmul(wt.nn, wl.tn));
    const cd n = Lo ? cadd(cneg(cmul(inc.nn, wt.tn)), cmul(wt.nn, inc.tn)) : cadd(cneg(cmul(wl.nn, inc.tn)), cmul(inc.nn, wl.tn));
    return cdiv(n, d);
}

// one interface of the ray tube.  (dx, dz) in at speed c, (ox, oz) out at speed oc; (nx, nz) the interface normal, curv the rate of
// turn of that normal per arc length along (nz, -nx); W / Th the tube's width / direction per radian of launch angle.
__device__ __forceinline__ void amp_tube_step(double dx, double dz, double c, double ox, double oz, double oc, double nx, double nz,
                                              double curv, bool refl, double& W, double& Th, double& prod)
{
    double cin = dx * nx + dz * nz;
    const double sg = cin < 0.0 ? -1.0 : 1.0;                  // the normal oriented along the incoming ray
    cin *= sg;
    const double cout = (ox * nx + oz * nz) * sg * (refl ? -1.0 : 1.0);
    const double K = curv * sg;
    const double ds = W / cin;
    const double dtin = Th - K * ds;
    const double dtout = (oc * cin) / (c * cout) * dtin;
    W = (refl ? -ds : ds) * cout;
    Th = refl ? K * ds - dtout : K * ds + dtout;
    prod = prod * cout / cin;
}

// ---- one leg as a path, element towards point: n unit segments, an interface between each two.  The kernels fill it from their own
// geometry (units and lengths are theirs: the walker never recomputes them) and amp_walk carries the tube and the coefficients along
// it in either direction: the up leg IS the down leg walked from its other end with negated directions.
#define AMP_MAX_SEG 4
enum AmpKind { AMP_INTO_SOLID, AMP_INTO_FLUID, AMP_FREE };   // what the path, element towards point, does at an interface
struct AmpSeg { double ux, uz, l, c, ic; bool L; };          // unit direction, length, speed, 1 / speed; in a solid: the mode is L
struct AmpIface {
    double nx, nz, curv;       // the normal and its rate of turn (amp_tube_step's convention)
    double tx, tz;             // the tangent of the coefficient frame
    AmpKind kind;
    const AmpMedia* m;         // the fluid-solid pair that meets here
};
struct AmpPath { int n; AmpSeg s[AMP_MAX_SEG]; AmpIface f[AMP_MAX_SEG - 1]; };

// leg 0..5 = L, T, LL, LT, TL, TT: a skip leg reflects once; the modes before (LX) and after it (LY)
__device__ __forceinline__ void amp_leg_modes(int leg, bool& skip, bool& LX, bool& LY)
{
    skip = leg >= 2;
    LX = leg == 0 || leg == 2 || leg == 3;
    LY = skip ? (leg == 2 || leg == 4) : LX;
}

// the ray crosses f from segment a into segment b (back: against the path, both directions negated): the tube's step, and the
// displacement coefficient at the tangential slowness of the arriving ray
__device__ __forceinline__ cd amp_cross(const AmpIface& f, const AmpSeg& a, const AmpSeg& b, bool back, double& W, double& Th, double& prod)
{
    const double ax = back ? -a.ux : a.ux, az = back ? -a.uz : a.uz, bx = back ? -b.ux : b.ux, bz = back ? -b.uz : b.uz;
    amp_tube_step(ax, az, a.c, bx, bz, b.c, f.nx, f.nz, f.curv, f.kind == AMP_FREE, W, Th, prod);
    const double p = (ax * f.tx + az * f.tz) * a.ic;
    if (f.kind == AMP_FREE) return amp_free(a.L, b.L, p, *f.m);
    return (f.kind == AMP_INTO_SOLID) != back ? amp_fluid_solid(b.L, p, *f.m) : amp_solid_fluid(a.L, p, *f.m);
}

// A = conj(D C_0 C_1 [C_2] G) of the path, down (element -> point) or up (point -> element); width, fc: the element's directivity
__device__ __forceinline__ float2 amp_walk(const AmpPath& p, bool up, double width, double fc)
{
    double W = 0.0, Th = 1.0, prod = 1.0;
    cd c[AMP_MAX_SEG - 1];
    if (!up) {
        W += p.s[0].l * Th;
#pragma unroll
        for (int i = 0; i < AMP_MAX_SEG - 1; ++i)
            if (i + 1 < p.n) { c[i] = amp_cross(p.f[i], p.s[i], p.s[i + 1], false, W, Th, prod); W += p.s[i + 1].l * Th; }
    } else {
#pragma unroll
        for (int i = AMP_MAX_SEG - 2; i >= 0; --i)
            if (i + 1 < p.n) { W += p.s[i + 1].l * Th; c[i] = amp_cross(p.f[i], p.s[i + 1], p.s[i], true, W, Th, prod); }
        W += p.s[0].l * Th;
    }
    cd C = c[0];
#pragma unroll
    for (int i = 1; i < AMP_MAX_SEG - 1; ++i)
        if (i + 1 < p.n) C = cmul(C, c[i]);
    double D = 1.0;
    if (width > 0.0) {
        const double u = width * p.s[0].ux * fc * p.s[0].ic;     // w sin(theta_E) / lambda_1
        D = u == 0.0 ? 1.0 : sinpi(u) / (M_PI * u);
    }
    if (W == 0.0) return make_float2(INFINITY, INFINITY);        // a caustic: ray theory fails (include/rtus.h)
    const double G = sqrt(prod / fabs(W));
    return make_float2((float)(D * G * C.re), (float)(-(D * G * C.im)));    // the conjugate: the analytic signal's convention
}
