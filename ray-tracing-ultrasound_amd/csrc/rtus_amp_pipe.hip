// rtus_amp_pipe.hip — ray amplitude tables of the multi-view legs through the curved lens into the pipe wall (rtus_leg_amp_pipe).
// NOT IN THE REFERENCE; checked against tests/pipe_amplitude_numpy.py (itself checked against a finite-difference ray tube through the
// three curved interfaces, a closed-form point on the axis, reciprocity and mirror symmetry).  Definitions: include/rtus.h.
//
// A = conj(D C_lens C_outer [C_bore] G): no solve, the path's angles are inputs (alpha, beta, gamma from rtus_tt_pipe[_skip]).  One lane
// per (element, point), straight-line code: the lens point with P' and P'' (rtus_lens.h's h, h', h''), the points on the two circles,
// the unit segments, the plane-wave coefficients of rtus_amp.h at the three interfaces, the ray tube through three or four segments,
// the directivity.  32 B in and 8 B out per skip entry; no workspace.
//
// Determinism: an entry is a function of its own inputs only (no lane or workgroup dependence).
#include "rtus_amp.h"
#include "rtus_lens.h"

#pragma clang fp contract(off)

struct PipeAmpArgs {
    double phi_3, twoTc, C4A, inv2A;   // the lens surface (rtus_lens.h)
    double c1, c2, ic1, ic2;           // L speed in the lens, speed in the water, their inverses
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

// unit vector and length of (dx, dz)
__device__ __forceinline__ void amp_seg(double dx, double dz, double& ux, double& uz, double& l)
{
    const double d2 = dx * dx + dz * dz, r = rsqrt_r<double>(d2);
    l = d2 * r; ux = dx * r; uz = dz * r;
}

__global__ __launch_bounds__(RTUS_BLOCK) void rtus_leg_amp_pipe_kernel(PipeAmpArgs a)
{
    const int f = blockIdx.x * RTUS_BLOCK + threadIdx.x, e = blockIdx.y;
    if (f >= a.n_f) return;
    const size_t o = (size_t)e * a.n_f + f;
    const bool skip = a.leg >= 2;
    const bool LX = a.leg == 0 || a.leg == 2 || a.leg == 3;     // L, LL, LT: first mode L
    const bool LY = skip ? (a.leg == 2 || a.leg == 4) : LX;     // LL, TL: second mode L
    const double cX = LX ? a.wall.cl : a.wall.ct, cY = LY ? a.wall.cl : a.wall.ct;
    const double icX = LX ? a.icl : a.ict, icY = LY ? a.icl : a.ict;
    const double al = a.alpha[o], be = a.beta[o];
    const double ga = skip ? a.gamma[o] : 0.0;
    if (isnan(al) || isnan(be) || isnan(ga)) { a.amp[o] = make_float2(NAN, NAN); return; }
    if (al == a.a_lo || al == a.a_hi) { a.amp[o] = make_float2(0.0f, 0.0f); return; }   // a pinned lens leg refracts by no law
    const double xe = a.xe[e], ze = a.ze[e], xf = a.xf[f], zf = a.zf[f];
    // the lens surface at alpha: P, P', P''; normal towards the water, tangent tau = P' / |P'|, turning rate of the normal
    double s, c;
    sincos(al, &s, &c);
    const double B = a.phi_3 * c - a.twoTc, B1 = -a.phi_3 * s, B2 = -a.phi_3 * c;
    const double disc = B * B - a.C4A;
    const double rS = rsqrt_r<double>(disc), S = disc * rS, BrS = B * rS;
    const double h = -(B + S) * a.inv2A;
    const double h1 = -B1 * (1.0 + BrS) * a.inv2A;
    const double h2 = -(B2 * (1.0 + BrS) + B1 * B1 * rS * (1.0 - BrS * BrS)) * a.inv2A;
    const double px = h * s, pz = h * c;
    const double p1x = h1 * s + pz, p1z = h1 * c - px;
    const double p2x = h2 * s + 2.0 * h1 * c - px, p2z = h2 * c - 2.0 * h1 * s - pz;
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
    // segments of the leg, element towards point
    double u1x, u1z, l1, u2x, u2z, l2, u3x, u3z, l3, u4x = 0.0, u4z = 0.0, l4 = 0.0;
    amp_seg(px - xe, pz - ze, u1x, u1z, l1);
    amp_seg(qx - px, qz - pz, u2x, u2z, l2);
    if (skip) {
        amp_seg(rx - qx, rz - qz, u3x, u3z, l3);
        amp_seg(xf - rx, zf - rz, u4x, u4z, l4);
    } else {
        amp_seg(xf - qx, zf - qz, u3x, u3z, l3);
    }
    {
        // every segment crosses its interface in the propagating sense: out of the lens, into the wall, off the bore
        bool ray = u1x * nlx + u1z * nlz > 0.0 && u2x * nlx + u2z * nlz > 0.0;
        ray = ray && u2x * nqx + u2z * nqz < 0.0 && u3x * nqx + u3z * nqz < 0.0;
        if (skip) ray = ray && u3x * nrx + u3z * nrz < 0.0 && u4x * nrx + u4z * nrz > 0.0;
        if (!ray) { a.amp[o] = make_float2(0.0f, 0.0f); return; }
    }
    const double tqx = -nqz, tqz = nqx, tbx = -nrz, tbz = nrx;
    double W = 0.0, Th = 1.0, prod = 1.0;
    cd C;
    if (!a.up) {
        W += l1 * Th;
        amp_tube_step(u1x, u1z, a.c1, u2x, u2z, a.c2, nlx, nlz, Kl, false, W, Th, prod);
        W += l2 * Th;
        amp_tube_step(u2x, u2z, a.c2, u3x, u3z, cX, nqx, nqz, a.inv_ro, false, W, Th, prod);
        W += l3 * Th;
        if (skip) {
            amp_tube_step(u3x, u3z, cX, u4x, u4z, cY, nrx, nrz, a.inv_ri, true, W, Th, prod);
            W += l4 * Th;
        }
        C = amp_solid_fluid(true, (u1x * taux + u1z * tauz) * a.ic1, a.lens);
        C = cmul(C, amp_fluid_solid(LX, (u2x * tqx + u2z * tqz) * a.ic2, a.wall));
        if (skip) C = cmul(C, amp_free(LX, LY, (u3x * tbx + u3z * tbz) * icX, a.wall));
    } else {
        if (skip) {
            W += l4 * Th;
            amp_tube_step(-u4x, -u4z, cY, -u3x, -u3z, cX, nrx, nrz, a.inv_ri, true, W, Th, prod);
        }
        W += l3 * Th;
        amp_tube_step(-u3x, -u3z, cX, -u2x, -u2z, a.c2, nqx, nqz, a.inv_ro, false, W, Th, prod);
        W += l2 * Th;
        amp_tube_step(-u2x, -u2z, a.c2, -u1x, -u1z, a.c1, nlx, nlz, Kl, false, W, Th, prod);
        W += l1 * Th;
        C = amp_fluid_solid(true, -(u2x * taux + u2z * tauz) * a.ic2, a.lens);
        C = cmul(C, amp_solid_fluid(LX, -(u3x * tqx + u3z * tqz) * icX, a.wall));
        if (skip) C = cmul(C, amp_free(LY, LX, -(u4x * tbx + u4z * tbz) * icY, a.wall));
    }
    double D = 1.0;
    if (a.width > 0.0) {
        const double u = a.width * u1x * a.fc * a.ic1;           // w sin(theta_E) / lambda_1
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

hipError_t rtus_launch_leg_amp_pipe(const rtus_lens& L, double a_lo, double a_hi, const rtus_pipe& P, const rtus_pipe_media& M, int leg,
                                    int up, double width, double f_c, const double* xe, const double* ze, int n_e, const double* xf,
                                    const double* zf, int n_f, const double* alpha, const double* beta, const double* gamma, float* amp,
                                    hipStream_t s)
{
    const LensK kk = make_lens_k(L);
    PipeAmpArgs a;
    a.phi_3 = kk.phi_3; a.twoTc = kk.twoTc; a.C4A = kk.C4A; a.inv2A = 1.0 / kk.twoA;
    a.c1 = L.c1; a.c2 = L.c2; a.ic1 = 1.0 / L.c1; a.ic2 = 1.0 / L.c2;
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
