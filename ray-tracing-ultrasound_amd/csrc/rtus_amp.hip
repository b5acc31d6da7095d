// rtus_amp.hip — ray amplitude tables of the multi-view legs through a measured surface (rtus_leg_amp_surface).  NOT IN THE
// REFERENCE; checked against tests/amplitude_numpy.py (itself checked against a 40-digit mpmath solve of the boundary conditions, an
// energy balance, reciprocity and a finite-difference ray tube).  Definitions: include/rtus.h.
//
// A = conj(D C_S [C_B] G): no solve, the leg's points are inputs (x_entry, x_back from rtus_tt_surface[_skip]).  One lane per
// (element, point), straight-line code: the spline at x_entry (rtus_spline.h) and the segment directions here; the walk along them is
// rtus_amp.h's amp_walk, shared with rtus_amp_pipe.hip: the plane-wave coefficients by Cramer's rule on the boundary conditions (3 x 3
// at the surface, 2 x 2 at the backwall; complex because the other modes may be evanescent), the ray tube's width carried through the
// segments and interfaces, the directivity.  About 300 fp64 operations and 24 B of traffic per entry.
//
// Determinism: an entry is a function of its own inputs only (no lane or workgroup dependence).
#include "rtus_amp.h"
#include "rtus_spline.h"

#pragma clang fp contract(off)

struct AmpArgs {
    double x0, dx, inv_dx;
    const double* __restrict__ coef;   // [n_s - 1][4] (rtus_surface_setup_kernel)
    int n_s, n_e, n_f, leg, up;
    AmpMedia m;                        // couplant | part
    double ic1, icl, ict;              // 1 / c1, 1 / c_l, 1 / c_t
    double zb, width, fc;
    const double* __restrict__ xe;
    const double* __restrict__ ze;
    const double* __restrict__ xf;
    const double* __restrict__ zf;
    const double* __restrict__ xent;
    const double* __restrict__ xback;  // skip legs only
    float2* __restrict__ amp;          // [n_e][n_f]
};

// a segment along (dx, dz): unit vector and length by square root and divide
__device__ __forceinline__ AmpSeg amp_seg_div(double dx, double dz, double c, double ic, bool L)
{
    const double l = sqrt(dx * dx + dz * dz);
    return {dx / l, dz / l, l, c, ic, L};
}

__global__ __launch_bounds__(RTUS_BLOCK) void rtus_leg_amp_surface_kernel(AmpArgs a)
{
    const int f = blockIdx.x * RTUS_BLOCK + threadIdx.x, e = blockIdx.y;
    if (f >= a.n_f) return;
    const size_t o = (size_t)e * a.n_f + f;
    bool skip, LX, LY;
    amp_leg_modes(a.leg, skip, LX, LY);
    const double x = a.xent[o];
    const double xb = skip ? a.xback[o] : 0.0;
    if (isnan(x) || isnan(xb)) { a.amp[o] = make_float2(NAN, NAN); return; }
    const double xe = a.xe[e], ze = a.ze[e], xf = a.xf[f], zf = a.zf[f];
    // the surface at x (x lies on the extent): unit normal into the part, tangent, curvature
    double s, s1, s2;
    spline_eval(a.coef, a.n_s, a.x0, a.dx, a.inv_dx, x, s, s1, s2);
    const double N2 = 1.0 + s1 * s1, N = sqrt(N2);
    const double nx = -s1 / N, nz = 1.0 / N, tx = nz, tz = -nx;
    const double kap = s2 / (N2 * N);
    // the leg, element towards point: to the surface, on to the point or (skip) to the backwall and from there to the point
    AmpPath p;
    p.n = skip ? 3 : 2;
    p.s[0] = amp_seg_div(x - xe, s - ze, a.m.c1, a.ic1, true);
    p.s[1] = amp_seg_div((skip ? xb : xf) - x, (skip ? a.zb : zf) - s, LX ? a.m.cl : a.m.ct, LX ? a.icl : a.ict, LX);
    if (skip) p.s[2] = amp_seg_div(xf - xb, zf - a.zb, LY ? a.m.cl : a.m.ct, LY ? a.icl : a.ict, LY);
    p.f[0] = {nx, nz, -kap, tx, tz, AMP_INTO_SOLID, &a.m};
    p.f[1] = {0.0, 1.0, 0.0, 1.0, 0.0, AMP_FREE, &a.m};
    // a stationary path that does not cross the surface into the part is no ray
    if (!(p.s[0].ux * nx + p.s[0].uz * nz > 0.0 && p.s[1].ux * nx + p.s[1].uz * nz > 0.0)) { a.amp[o] = make_float2(0.0f, 0.0f); return; }
    a.amp[o] = amp_walk(p, a.up != 0, a.width, a.fc);
}

hipError_t rtus_launch_leg_amp_surface(double x0, double dx, const double* zs, int n_s, double c1, double rho1, double c_l, double c_t,
                                       double rho2, double z_back, int leg, int up, double width, double f_c, const double* xe,
                                       const double* ze, int n_e, const double* xf, const double* zf, int n_f, const double* x_entry,
                                       const double* x_back, float* amp, void* ws, hipStream_t s)
{
    AmpArgs a;
    a.x0 = x0; a.dx = dx; a.inv_dx = 1.0 / dx;
    a.n_s = n_s; a.n_e = n_e; a.n_f = n_f; a.leg = leg; a.up = up;
    a.m = {c1, rho1, c_l, c_t, rho2};
    a.ic1 = 1.0 / c1; a.icl = 1.0 / c_l; a.ict = 1.0 / c_t;
    a.zb = z_back; a.width = width; a.fc = f_c;
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
