// rtus_amp.hip — ray amplitude tables of the multi-view legs through a measured surface (rtus_leg_amp_surface).  NOT IN THE
// REFERENCE; checked against tests/amplitude_numpy.py (itself checked against a 40-digit mpmath solve of the boundary conditions, an
// energy balance, reciprocity and a finite-difference ray tube).  Definitions: include/rtus.h.
//
// A = conj(D C_S [C_B] G): no solve, the leg's points are inputs (x_entry, x_back from rtus_tt_surface[_skip]).  One lane per
// (element, point), straight-line code: the spline at x_entry, the segment directions, the plane-wave coefficients by Cramer's rule on
// the boundary conditions (3 x 3 at the surface, 2 x 2 at the backwall; complex because the other modes may be evanescent), the ray
// tube's width carried through the segments and interfaces, the directivity.  About 300 fp64 operations and 24 B of traffic per entry.
//
// Determinism: an entry is a function of its own inputs only (no lane or workgroup dependence).
#include "rtus_amp.h"

#pragma clang fp contract(off)

struct AmpArgs {
    double x0, dx, inv_dx;
    const double* __restrict__ coef;   // [n_s - 1][4] (rtus_surface_setup_kernel)
    int n_s, n_e, n_f, leg, up;
    double c1, r1, cl, ct, r2, zb, width, fc;
    const double* __restrict__ xe;
    const double* __restrict__ ze;
    const double* __restrict__ xf;
    const double* __restrict__ zf;
    const double* __restrict__ xent;
    const double* __restrict__ xback;  // skip legs only
    float2* __restrict__ amp;          // [n_e][n_f]
};

__global__ __launch_bounds__(RTUS_BLOCK) void rtus_leg_amp_surface_kernel(AmpArgs a)
{
    const int f = blockIdx.x * RTUS_BLOCK + threadIdx.x, e = blockIdx.y;
    if (f >= a.n_f) return;
    const size_t o = (size_t)e * a.n_f + f;
    const bool skip = a.leg >= 2;
    const bool LX = a.leg == 0 || a.leg == 2 || a.leg == 3;     // L, LL, LT: first mode L
    const bool LY = skip ? (a.leg == 2 || a.leg == 4) : LX;     // LL, TL: second mode L
    const double cX = LX ? a.cl : a.ct, cY = LY ? a.cl : a.ct;
    const double x = a.xent[o];
    const double xb = skip ? a.xback[o] : 0.0;
    if (isnan(x) || isnan(xb)) { a.amp[o] = make_float2(NAN, NAN); return; }
    const double xe = a.xe[e], ze = a.ze[e], xf = a.xf[f], zf = a.zf[f];
    // the spline at x (tests/surface_numpy.py's segment rule; x lies on the extent)
    double kf = floor((x - a.x0) * a.inv_dx);
    kf = !(kf >= 0.0) ? 0.0 : (kf > (double)(a.n_s - 2) ? (double)(a.n_s - 2) : kf);
    const int k = (int)kf;
    const double t = x - fma(kf, a.dx, a.x0);
    const double c0 = a.coef[4 * k], c1 = a.coef[4 * k + 1], c2 = a.coef[4 * k + 2], c3 = a.coef[4 * k + 3];
    const double s = fma(fma(fma(c3, t, c2), t, c1), t, c0);
    const double s1 = fma(fma(3.0 * c3, t, 2.0 * c2), t, c1);
    const double s2 = fma(6.0 * c3, t, 2.0 * c2);
    const double N2 = 1.0 + s1 * s1, N = sqrt(N2);
    const double nx = -s1 / N, nz = 1.0 / N, tx = nz, tz = -nx;
    const double kap = s2 / (N2 * N);
    // segments of the leg, element towards point
    double ux = x - xe, uz = s - ze;
    const double l1 = sqrt(ux * ux + uz * uz);
    ux /= l1; uz /= l1;
    double bx = 0.0, bz = 0.0, l2, l3 = 0.0, fx, fz;
    if (skip) {
        bx = xb - x; bz = a.zb - s;
        l2 = sqrt(bx * bx + bz * bz);
        bx /= l2; bz /= l2;
        fx = xf - xb; fz = zf - a.zb;
        l3 = sqrt(fx * fx + fz * fz);
        fx /= l3; fz /= l3;
    } else {
        fx = xf - x; fz = zf - s;
        l2 = sqrt(fx * fx + fz * fz);
        fx /= l2; fz /= l2;
    }
    {
        const double ox = skip ? bx : fx, oz = skip ? bz : fz;  // a stationary path that does not cross the surface into the part
        if (!(ux * nx + uz * nz > 0.0 && ox * nx + oz * nz > 0.0)) { a.amp[o] = make_float2(0.0f, 0.0f); return; }
    }
    double W = 0.0, Th = 1.0, prod = 1.0;
    cd C;
    if (!a.up) {
        W += l1 * Th;
        const double ox = skip ? bx : fx, oz = skip ? bz : fz;
        amp_tube_step(ux, uz, a.c1, ox, oz, cX, nx, nz, -kap, false, W, Th, prod);
        W += l2 * Th;
        if (skip) {
            amp_tube_step(bx, bz, cX, fx, fz, cY, 0.0, 1.0, 0.0, true, W, Th, prod);
            W += l3 * Th;
        }
        C = amp_fluid_solid(LX, (ux * tx + uz * tz) / a.c1, a);
        if (skip) C = cmul(C, amp_free(LX, LY, bx / cX, a));
    } else {
        double ix, iz;                                           // the ray arriving at the surface from below
        if (skip) {
            W += l3 * Th;
            amp_tube_step(-fx, -fz, cY, -bx, -bz, cX, 0.0, 1.0, 0.0, true, W, Th, prod);
            W += l2 * Th;
            ix = -bx; iz = -bz;
        } else {
            W += l2 * Th;
            ix = -fx; iz = -fz;
        }
        amp_tube_step(ix, iz, cX, -ux, -uz, a.c1, nx, nz, -kap, false, W, Th, prod);
        W += l1 * Th;
        C = amp_solid_fluid(LX, (ix * tx + iz * tz) / cX, a);
        if (skip) C = cmul(C, amp_free(LY, LX, -fx / cY, a));
    }
    double D = 1.0;
    if (a.width > 0.0) {
        const double u = a.width * ux * a.fc / a.c1;             // w sin(theta_E) / lambda_1
        D = u == 0.0 ? 1.0 : sinpi(u) / (M_PI * u);
    }
    float2 r;
    if (W == 0.0) {
        r = make_float2(INFINITY, INFINITY);                     // a caustic: ray theory fails (include/rtus.h)
    } else {
        const double G = sqrt(prod / fabs(W));
        r = make_float2((float)(D * G * C.re), (float)(-(D * G * C.im)));   // the conjugate: the analytic signal's convention
    }
    a.amp[o] = r;
}

hipError_t rtus_launch_surface_setup(const double* zs, int n_s, double x0, double dx, void* ws, const double** coef, hipStream_t s);

hipError_t rtus_launch_leg_amp_surface(double x0, double dx, const double* zs, int n_s, double c1, double rho1, double c_l, double c_t,
                                       double rho2, double z_back, int leg, int up, double width, double f_c, const double* xe,
                                       const double* ze, int n_e, const double* xf, const double* zf, int n_f, const double* x_entry,
                                       const double* x_back, float* amp, void* ws, hipStream_t s)
{
    AmpArgs a;
    a.x0 = x0; a.dx = dx; a.inv_dx = 1.0 / dx;
    a.n_s = n_s; a.n_e = n_e; a.n_f = n_f; a.leg = leg; a.up = up;
    a.c1 = c1; a.r1 = rho1; a.cl = c_l; a.ct = c_t; a.r2 = rho2; a.zb = z_back; a.width = width; a.fc = f_c;
    a.xe = xe; a.ze = ze; a.xf = xf; a.zf = zf; a.xent = x_entry; a.xback = x_back; a.amp = (float2*)amp;
    const long long gx = ((long long)n_f + RTUS_BLOCK - 1) / RTUS_BLOCK;
    if (n_e > 65535 || gx > 0x7fffffffLL) return hipErrorInvalidValue;
    const double* coef = nullptr;
    hipError_t e = rtus_launch_surface_setup(zs, n_s, x0, dx, ws, &coef, s);
    if (e != hipSuccess) return e;
    a.coef = coef;
    hipLaunchKernelGGL(rtus_leg_amp_surface_kernel, dim3((unsigned)gx, (unsigned)n_e), dim3(RTUS_BLOCK), 0, s, a);
    return hipGetLastError();
}
