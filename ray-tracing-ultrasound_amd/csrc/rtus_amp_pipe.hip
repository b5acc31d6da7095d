// rtus_amp_pipe.hip — ray amplitude tables of the multi-view legs through the curved lens into the pipe wall (rtus_leg_amp_pipe).
// NOT IN THE REFERENCE; checked against tests/pipe_amplitude_numpy.py (itself checked against a finite-difference ray tube through the
// three curved interfaces, a closed-form point on the axis, reciprocity and mirror symmetry).  Definitions: include/rtus.h.
//
// A = conj(D C_lens C_outer [C_bore] G): no solve, the path's angles are inputs (alpha, beta, gamma from rtus_tt_pipe[_skip]).  One lane
// per (element, point), straight-line code: the lens point with P' and P'' (rtus_lens.h's lens_point), the points on the two circles
// and the unit segments here; the walk along them is rtus_amp.h's amp_walk, shared with rtus_amp.hip: the plane-wave coefficients at
// the three interfaces, the ray tube through three or four segments, the directivity.  32 B in and 8 B out per skip entry; no workspace.
//
// Determinism: an entry is a function of its own inputs only (no lane or workgroup dependence).
#include "rtus_amp.h"
#include "rtus_lens.h"

#pragma clang fp contract(off)

struct PipeAmpArgs {
    LensConst<double> k;               // the lens surface (rtus_lens.h); c1inv, c2inv: 1 / the speeds below
    double c1, c2;                     // L speed in the lens, speed in the water
    double a_lo, a_hi;
    double r_out, r_in, inv_ro, inv_ri, x_off;
    AmpMedia lens, wall;               // water | lens, water | wall
    double icl, ict;                   // 1 / c_l, 1 / c_t of the wall
    double width, fc;
    int n_e, n_f, leg, up;
    const double* __restrict__ xe;
    const double* __restrict__ ze;
    const double* __restrict__ xf;
    const double* __restrict__ zf;
    const double* __restrict__ alpha;
    const double* __restrict__ beta;
    const double* __restrict__ gamma;  // skip legs only
    float2* __restrict__ amp;          // [n_e][n_f]
};

// a segment along (dx, dz): unit vector and length by reciprocal square root
__device__ __forceinline__ AmpSeg amp_seg_rsq(double dx, double dz, double c, double ic, bool L)
{
    const double d2 = dx * dx + dz * dz, r = rsqrt_r<double>(d2);
    return {dx * r, dz * r, d2 * r, c, ic, L};
}

__global__ __launch_bounds__(RTUS_BLOCK) void rtus_leg_amp_pipe_kernel(PipeAmpArgs a)
{
    const int f = blockIdx.x * RTUS_BLOCK + threadIdx.x, e = blockIdx.y;
    if (f >= a.n_f) return;
    const size_t o = (size_t)e * a.n_f + f;
    bool skip, LX, LY;
    amp_leg_modes(a.leg, skip, LX, LY);
    const double al = a.alpha[o], be = a.beta[o];
    const double ga = skip ? a.gamma[o] : 0.0;
    if (isnan(al) || isnan(be) || isnan(ga)) { a.amp[o] = make_float2(NAN, NAN); return; }
    if (al == a.a_lo || al == a.a_hi) { a.amp[o] = make_float2(0.0f, 0.0f); return; }   // a pinned lens leg refracts by no law
    const double xe = a.xe[e], ze = a.ze[e], xf = a.xf[f], zf = a.zf[f];
    // the lens surface at alpha: normal towards the water, tangent tau = P' / |P'|, turning rate of the normal
    double px, pz, p1x, p1z, p2x, p2z;
    lens_point<false, true>(a.k, al, px, pz, p1x, p1z, p2x, p2z);
    const double rp = rsqrt_r<double>(p1x * p1x + p1z * p1z);
    const double taux = p1x * rp, tauz = p1z * rp;
    const double nlx = tauz, nlz = -taux;
    const double Kl = (p1x * p2z - p1z * p2x) * (rp * rp * rp);
    // the outer circle at beta, the bore at gamma: outward normals; the coefficient frames' tangents are those of the inward ones
    double nqx, nqz, nrx = 0.0, nrz = 1.0;
    sincos(be, &nqx, &nqz);
    const double qx = fma(a.r_out, nqx, a.x_off), qz = a.r_out * nqz;
    double rx = 0.0, rz = 0.0;
    if (skip) {
        sincos(ga, &nrx, &nrz);
        rx = fma(a.r_in, nrx, a.x_off); rz = a.r_in * nrz;
    }
    // the leg, element towards point: through the lens, the water, the wall to the point or (skip) to the bore and from there to the point
    AmpPath p;
    p.n = skip ? 4 : 3;
    p.s[0] = amp_seg_rsq(px - xe, pz - ze, a.c1, a.k.c1inv, true);
    p.s[1] = amp_seg_rsq(qx - px, qz - pz, a.c2, a.k.c2inv, true);
    p.s[2] = amp_seg_rsq((skip ? rx : xf) - qx, (skip ? rz : zf) - qz, LX ? a.wall.cl : a.wall.ct, LX ? a.icl : a.ict, LX);
    if (skip) p.s[3] = amp_seg_rsq(xf - rx, zf - rz, LY ? a.wall.cl : a.wall.ct, LY ? a.icl : a.ict, LY);
    p.f[0] = {nlx, nlz, Kl, taux, tauz, AMP_INTO_FLUID, &a.lens};
    p.f[1] = {nqx, nqz, a.inv_ro, -nqz, nqx, AMP_INTO_SOLID, &a.wall};
    p.f[2] = {nrx, nrz, a.inv_ri, -nrz, nrx, AMP_FREE, &a.wall};
    {
        // every segment crosses its interface in the propagating sense: out of the lens, into the wall, off the bore
        bool ray = p.s[0].ux * nlx + p.s[0].uz * nlz > 0.0 && p.s[1].ux * nlx + p.s[1].uz * nlz > 0.0;
        ray = ray && p.s[1].ux * nqx + p.s[1].uz * nqz < 0.0 && p.s[2].ux * nqx + p.s[2].uz * nqz < 0.0;
        if (skip) ray = ray && p.s[2].ux * nrx + p.s[2].uz * nrz < 0.0 && p.s[3].ux * nrx + p.s[3].uz * nrz > 0.0;
        if (!ray) { a.amp[o] = make_float2(0.0f, 0.0f); return; }
    }
    a.amp[o] = amp_walk(p, a.up != 0, a.width, a.fc);
}

hipError_t rtus_launch_leg_amp_pipe(const rtus_lens& L, double a_lo, double a_hi, const rtus_pipe& P, const rtus_pipe_media& M, int leg,
                                    int up, double width, double f_c, const double* xe, const double* ze, int n_e, const double* xf,
                                    const double* zf, int n_f, const double* alpha, const double* beta, const double* gamma, float* amp,
                                    hipStream_t s)
{
    PipeAmpArgs a;
    a.k = make_lens_const<double>(L, a_lo, a_hi);
    a.c1 = L.c1; a.c2 = L.c2;
    a.a_lo = a_lo; a.a_hi = a_hi;
    a.r_out = P.r_outer; a.r_in = P.r_inner; a.inv_ro = 1.0 / P.r_outer; a.inv_ri = P.r_inner > 0 ? 1.0 / P.r_inner : 0.0;
    a.x_off = P.x_off;
    a.lens = {L.c2, M.rho_water, L.c1, M.ct_lens, M.rho_lens};
    a.wall = {L.c2, M.rho_water, M.c_l, M.c_t, M.rho_wall};
    a.icl = 1.0 / M.c_l; a.ict = 1.0 / M.c_t;
    a.width = width; a.fc = f_c;
    a.n_e = n_e; a.n_f = n_f; a.leg = leg; a.up = up;
    a.xe = xe; a.ze = ze; a.xf = xf; a.zf = zf; a.alpha = alpha; a.beta = beta; a.gamma = gamma; a.amp = (float2*)amp;
    const long long gx = ((long long)n_f + RTUS_BLOCK - 1) / RTUS_BLOCK;
    if (n_e > 65535 || gx > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rtus_leg_amp_pipe_kernel, dim3((unsigned)gx, (unsigned)n_e), dim3(RTUS_BLOCK), 0, s, a);
    return hipGetLastError();
}
