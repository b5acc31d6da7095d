// rtus_spline.h — the measured surface's natural cubic spline as the kernels read it, and the set-up that makes it (rtus_surface.hip),
// for the table kernels there and for the consumers of a surface table in other files (rtus_amp.hip).
#pragma once
#include "rtus_device.h"

// no implicit contraction (as in both users): the fma()s are written out
#pragma clang fp contract(off)

// bytes of a surface workspace for n_s samples (the spline's coefficients, the scan points, the depth extremes)
size_t rtus_surface_ws_bytes(int n_s);
// the set-up kernel alone: the spline's coefficients [n_s - 1][4] land in the workspace at *coef (the scan points are written too, as
// for a table launch)
hipError_t rtus_launch_surface_setup(const double* zs, int n_s, double x0, double dx, void* ws, const double** coef, hipStream_t s);
// ... for a table kernel in another file (rtus_aniso.hip): also where the set-up leaves the m scan points P_j = x0 + j dx / 4 as
// fp32 (x - xo, s - zo, s', 0) and the profile's least and greatest depth (smin[0], smin[1])
struct RtusSurfaceScan {
    const double* coef;
    const float4* pts;
    const double* smin;
    double xo, zo;
    int m;
};
hipError_t rtus_launch_surface_setup_scan(const double* zs, int n_s, double x0, double dx, void* ws, RtusSurfaceScan* scan, hipStream_t s);

// s, s', s'' at x (x clamped to the extent's segments: outside it the end segments' cubics continue)
__device__ __forceinline__ void spline_eval(const double* __restrict__ coef, int n_s, double x0, double dx, double inv_dx, double x,
                                            double& s, double& s1, double& s2)
{
    double kf = floor((x - x0) * inv_dx);
    kf = !(kf >= 0.0) ? 0.0 : (kf > (double)(n_s - 2) ? (double)(n_s - 2) : kf);       // (NaN -> segment 0: never out of bounds)
    const int k = (int)kf;
    const double t = x - fma(kf, dx, x0);
    const double a = coef[4 * k], b = coef[4 * k + 1], c = coef[4 * k + 2], d = coef[4 * k + 3];
    s = fma(fma(fma(d, t, c), t, b), t, a);
    s1 = fma(fma(3.0 * d, t, 2.0 * c), t, b);
    s2 = fma(6.0 * d, t, 2.0 * c);
}
