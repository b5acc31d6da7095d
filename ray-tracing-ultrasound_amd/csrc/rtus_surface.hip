// rtus_surface.hip — element x focal-point Fermat travel times through ONE curved interface given as a sampled depth
// profile (natural cubic spline through zs[k] at x0 + k dx).  NOT IN THE REFERENCE (parity unpinned): checked against
// tests/surface_numpy.py (itself checked against mpmath) and, on a flat profile, against the planar solver.
//
// T(x) = |E - S(x)| / c1 + |S(x) - F| / c2,  S(x) = (x, s(x));  the entry is the least T over the interior local minima of T.
//
//   1. rtus_surface_setup_kernel (one workgroup): the spline's second derivatives (Thomas solve of the natural-spline system,
//      one lane: n_s - 2 unknowns), the per-segment cubic coefficients, the profile's minimum depth and the scan points
//      P_j = x0 + j dx / 4, j = 0 .. 4 (n_s - 1), as fp32 (x, s, s') relative to the profile's centre — all into the caller's
//      workspace, on the stream (graph-capturable).
//   2. rtus_surface_kernel: lanes are consecutive focal points, a workgroup owns SURF_EB elements.  A local minimum of T is a
//      sign change - -> + of T'(x) = g1(x) / c1 + g2(x) / c2, g_i = (unit vector from the surface point to E / F) . (1, s'),
//      so the scan tests the SIGN of T' at every P_j:  g2 (the focal point's term: one v_rsq_f32 per lane and point) is shared
//      by the workgroup's elements, -(c2 / c1) g1 (the element's term) is computed once per (element, point) into LDS and read
//      as a broadcast.  Per (element, point) that is one compare plus lane-mask logic on the scalar unit; a lane whose sign
//      goes from - to + ranks the bracket [P_j, P_j+1] by an fp32 lower bound of its minimum's T (step 3) and keeps the SURF_K best.
//   3. The kept brackets are refined in fp64: safeguarded Newton (bisection when a step leaves the bracket or T'' <= 0) on
//      T'(x) = 0 with the cubic's analytic s' and s''.  The entry is the least refined time.  Where the fp32 sign at a bracket
//      end was wrong (|T'| below fp32 resolution: within ~1e-8 m of the root) the fp64 signs pick the neighbouring interval
//      instead.  The first two are refined always, the third unless it cannot win: the scan's figure for a bracket is a LOWER
//      BOUND of its minimum's time, T(P_j+1) - (dx / 4) T'(P_j+1) at the bracket's right scan point (T' grows from 0 at the
//      root to T'(P_j+1) over less than dx / 4: exact where T' is monotone there, and where T'' is linear as long as the next
//      stationary point is dx / 2 away), and the third bracket is skipped when its bound is later than the best REFINED time by
//      more than the fp32 error of the bound (4e-6 relative).  (T(P_j+1) itself is above the minimum's time by up to
//      T'' (dx / 4)^2 / 2, ~1e-8 s on a 1 mm grid, a different amount for each bracket: a third bracket skipped on that figure
//      against the best such figure — as it was — loses the entry's least minimum where three minima lie within that error of
//      each other: DESIGN.md, tests/test_gpu_surface_branches.py.)
//
// Guarantee: a minimum whose neighbouring stationary points are at least dx / 2 away on both sides (the ends of the extent do
// not count) has a scan point in its decreasing part and the next one in its increasing part (spacing dx / 4: a quarter of
// margin for the fp32 signs) and is bracketed; the entry is the least T over such minima WHERE THE ENTRY HAS AT MOST SURF_K = 3
// BRACKETS.  With four or more, the fourth and later are still dropped on the scan's figure (the three least bounds are kept):
// the least minimum can be dropped where its time is within T'' (dx / 4)^2 of the third kept one's, and the entry is then late
// by at most that.  Narrower minima may be missed.  Either can only make the entry later (or NaN).
//
// Determinism: every value an entry is made of is computed from its own element, focal point, the profile and the speeds,
// by code that does not depend on the element's slot in the workgroup or on the lane: the entry has the same bits whatever
// else shares the call.
//
// Plane waves (rtus_pw_surface): the same kernel with ANGLES in the elements' place (template argument SURF_PW).  The first leg is
// the plane wave's time to S(x), ((x - x_ref) sin t + (s(x) - z_a) cos t) / c1, so -(c2 / c1) g1 becomes -(c2 / c1)(sin t +
// s' cos t) and T'' loses the first leg's curvature term (s'' cos t / c1 remains).  Only entry points whose ray traced back
// along the incident direction meets the aperture count (insonified): an out-of-band scan point carries NaN in LDS and never
// becomes the "-" side of a bracket (a NaN term would otherwise read as - and fake a - -> + change at every band edge), and the
// refined root is tested against the band in fp64.
//
// Skip legs (rtus_tt_surface_skip, SURF_SKIP): elements as in SURF_ELEM, the leg below the surface reflected once off a planar
// backwall at zb (down at c_down = c2, up at c_up).  Only the lane term changes: per scan point the lane solves the leg below the
// surface for its horizontal slowness (u = c_down p, SKIP_NEWTON safeguarded fp32 Newton steps warm-started from the previous
// scan point) and tests -(u + a_d s') > ng (T_in' = -(p + q_d s'), envelope theorem); the bracket estimate is T_in + st1.  The
// refine solves u to convergence in fp64 (skip_inner) inside surf_T_skip.  The set-up kernel also reduces max s (smin[1]) for
// the rule zb > max s.
//
// The kept triple, the fp64 bracket of step 3 and its Newton are rtus_bracket.h's, shared with rtus_lens_pipe.hip.
#include "rtus_device.h"
#include "rtus_bracket.h"
#include "rtus_spline.h"    // spline_eval; rtus_surface_ws_bytes and rtus_launch_surface_setup, defined here

// no implicit contraction: the fma()s are written out, so every element slot's inlined copy of the arithmetic rounds alike
#pragma clang fp contract(off)

#define SURF_EB 8           // elements per workgroup (register block: the focal point's leg is shared by them)
#define SURF_TILE 64        // scan points per LDS tile
#define SURF_K 3            // brackets kept per (element, focal point)
#define SURF_SUB 4          // scan points per profile segment

struct SurfArgs {
    double x0, dx, hq, inv_dx, xend;   // hq = dx / SURF_SUB
    double c1, c2, xo, zo;             // (xo, zo): origin of the fp32 scan coordinates
    float ic1f, ic2f, k21f, hqic2f;    // 1 / c1, 1 / c2, c2 / c1, hq / c2
    int n_s, m, n_e, n_f;
    const double* __restrict__ xe;
    const double* __restrict__ ze;
    const double* __restrict__ xf;
    const double* __restrict__ zf;
    double* __restrict__ tt;
    double* __restrict__ xent;         // nullable
    const double* __restrict__ coef;   // [n_s - 1][4]: a, b, c, d of s(x0 + k dx + t) = a + b t + c t^2 + d t^3
    const float4* __restrict__ pts;    // [m]: (x - xo, s - zo, s', 0)
    const double* __restrict__ smin;   // the profile's least depth (smin[1]: its greatest)
    // plane waves (PW instantiation): n_e counts angles; the aperture [x_lo, x_hi] at depth z_a
    const double* __restrict__ ang;
    double xlo, xhi, za;
    // skip legs (SKIP instantiation): c2 is c_down; the backwall at zb, kap = c_down / c_up, umax = min(1, kap)
    double zb, kap, umax;
    float zbr, kap2f, umaxf;           // zb - zo, kap^2, umax less a margin (fp32 scan)
    double* __restrict__ xback;        // nullable
};

// workspace layout (256-byte aligned pieces): M [n_s] | Thomas scratch [n_s] | coef [4 (n_s - 1)] | pts [m] | smin, smax
static inline __host__ __device__ int surf_points(int n_s) { return SURF_SUB * (n_s - 1) + 1; }
size_t rtus_surface_ws_bytes(int n_s)
{
    return 2 * rtus_al256(8 * (size_t)n_s) + rtus_al256(32 * (size_t)(n_s - 1)) + rtus_al256(16 * (size_t)surf_points(n_s)) + 256;
}

struct SurfWs {
    double *M, *cp, *coef, *smin;
    float4* pts;
};
static SurfWs surf_ws(void* ws, int n_s)
{
    char* p = (char*)ws;
    SurfWs w;
    w.M = (double*)p;  p += rtus_al256(8 * (size_t)n_s);
    w.cp = (double*)p; p += rtus_al256(8 * (size_t)n_s);
    w.coef = (double*)p; p += rtus_al256(32 * (size_t)(n_s - 1));
    w.pts = (float4*)p; p += rtus_al256(16 * (size_t)surf_points(n_s));
    w.smin = (double*)p;
    return w;
}

__global__ void __launch_bounds__(RTUS_BLOCK) rtus_surface_setup_kernel(const double* __restrict__ zs, int n_s, double x0, double dx,
                                                                          double xo, double zo, SurfWs w)
{
    const int tid = threadIdx.x;
    // natural spline: M_0 = M_{n-1} = 0,  M_{i-1} + 4 M_i + M_{i+1} = 6 (z_{i+1} - 2 z_i + z_{i-1}) / dx^2
    if (tid == 0) {
        const double r6 = 6.0 / (dx * dx);
        double cprev = 0.0, dprev = 0.0;
        for (int i = 1; i <= n_s - 2; ++i) {
            const double rhs = r6 * ((zs[i + 1] - zs[i]) - (zs[i] - zs[i - 1]));
            const double inv = 1.0 / (4.0 - cprev);
            cprev = inv;
            dprev = (rhs - dprev) * inv;
            w.cp[i] = cprev;
            w.M[i] = dprev;
        }
        w.M[0] = 0.0;
        w.M[n_s - 1] = 0.0;
        for (int i = n_s - 3; i >= 1; --i) w.M[i] = fma(-w.cp[i], w.M[i + 1], w.M[i]);
    }
    __syncthreads();
    __shared__ double red[RTUS_BLOCK], red_hi[RTUS_BLOCK];
    double lo = INFINITY, up = -INFINITY;
    for (int k = tid; k < n_s - 1; k += RTUS_BLOCK) {
        const double Mk = w.M[k], Mk1 = w.M[k + 1], z0 = zs[k], z1 = zs[k + 1];
        const double a = z0, b = (z1 - z0) / dx - dx * (2.0 * Mk + Mk1) / 6.0, c = 0.5 * Mk, d = (Mk1 - Mk) / (6.0 * dx);
        w.coef[4 * k] = a; w.coef[4 * k + 1] = b; w.coef[4 * k + 2] = c; w.coef[4 * k + 3] = d;
        // least depth on the segment: its ends and the roots of s' = b + 2 c t + 3 d t^2 inside it
        const double zend = fma(fma(fma(d, dx, c), dx, b), dx, a);
        double m = fmin(a, zend), mx = fmax(a, zend);
        const double A = 3.0 * d, B = 2.0 * c, disc = B * B - 4.0 * A * b;
        double r[2] = {NAN, NAN};
        if (A != 0.0) {
            if (disc >= 0.0) { const double q = sqrt(disc); r[0] = (-B - q) / (2.0 * A); r[1] = (-B + q) / (2.0 * A); }
        } else if (B != 0.0) {
            r[0] = -b / B;
        }
        for (int i = 0; i < 2; ++i)
            if (r[i] > 0.0 && r[i] < dx) {
                const double zr = fma(fma(fma(d, r[i], c), r[i], b), r[i], a);
                m = fmin(m, zr);
                mx = fmax(mx, zr);
            }
        lo = fmin(lo, m);
        up = fmax(up, mx);
    }
    red[tid] = lo;
    red_hi[tid] = up;
    __syncthreads();
    for (int h = RTUS_BLOCK / 2; h > 0; h >>= 1) {
        if (tid < h) { red[tid] = fmin(red[tid], red[tid + h]); red_hi[tid] = fmax(red_hi[tid], red_hi[tid + h]); }
        __syncthreads();
    }
    if (tid == 0) { w.smin[0] = red[0]; w.smin[1] = red_hi[0]; }     // least and greatest depth (the slot holds 256 bytes)
    const int m = surf_points(n_s);
    const double hq = dx / SURF_SUB;
    for (int j = tid; j < m; j += RTUS_BLOCK) {
        const int k = j / SURF_SUB < n_s - 2 ? j / SURF_SUB : n_s - 2;
        const double t = (double)(j - SURF_SUB * k) * hq;
        const double* cf = w.coef + 4 * k;
        const double s = fma(fma(fma(cf[3], t, cf[2]), t, cf[1]), t, cf[0]);
        const double s1 = fma(fma(3.0 * cf[3], t, 2.0 * cf[2]), t, cf[1]);
        w.pts[j] = make_float4((float)(fma((double)j, hq, x0) - xo), (float)(s - zo), (float)s1, 0.0f);
    }
}

// T'(x) and T''(x) (and T) in fp64
struct Tder { double t, d1, d2; };
__device__ __forceinline__ Tder surf_T(const double* __restrict__ coef, int n_s, double x0, double dx, double inv_dx, double inv_c1,
                                       double inv_c2, double xe, double ze, double xf, double zf, double x)
{
    double s, s1, s2;
    spline_eval(coef, n_s, x0, dx, inv_dx, x, s, s1, s2);
    const double ux = x - xe, uz = s - ze, vx = x - xf, vz = s - zf;
    const double q1 = fma(ux, ux, uz * uz), q2 = fma(vx, vx, vz * vz);
    const double r1 = 1.0 / sqrt(q1), r2 = 1.0 / sqrt(q2);
    const double l1 = q1 * r1, l2 = q2 * r2;                     // the two leg lengths
    const double A1 = fma(uz, s1, ux), A2 = fma(vz, s1, vx);     // (S - E) . S',  (S - F) . S'
    const double B = fma(s1, s1, 1.0);                           // |S'|^2
    Tder o;
    o.t = fma(l1, inv_c1, l2 * inv_c2);
    o.d1 = fma(A1 * r1, inv_c1, A2 * r2 * inv_c2);
    o.d2 = fma((fma(uz, s2, B) - A1 * A1 * r1 * r1) * r1, inv_c1, (fma(vz, s2, B) - A2 * A2 * r2 * r2) * r2 * inv_c2);
    return o;
}

// the same for a plane wave: first leg ((x - x_ref) sn + (s - z_a) cs) / c1
__device__ __forceinline__ Tder surf_T_pw(const double* __restrict__ coef, int n_s, double x0, double dx, double inv_dx, double inv_c1,
                                          double inv_c2, double sn, double cs, double xref, double za, double xf, double zf, double x)
{
    double s, s1, s2;
    spline_eval(coef, n_s, x0, dx, inv_dx, x, s, s1, s2);
    const double vx = x - xf, vz = s - zf;
    const double q2 = fma(vx, vx, vz * vz);
    const double r2 = 1.0 / sqrt(q2);
    const double l2 = q2 * r2;
    const double A2 = fma(vz, s1, vx);
    const double B = fma(s1, s1, 1.0);
    Tder o;
    o.t = fma(fma(x - xref, sn, (s - za) * cs), inv_c1, l2 * inv_c2);
    o.d1 = fma(fma(s1, cs, sn), inv_c1, A2 * r2 * inv_c2);
    o.d2 = fma(s2 * cs, inv_c1, (fma(vz, s2, B) - A2 * A2 * r2 * r2) * r2 * inv_c2);
    return o;
}

// skip leg below the surface, in the down-going slowness scaled by c_down: u = c_down p, a_d = sqrt(1 - u^2), a_u = sqrt(kap^2 - u^2)
// (kap = c_down / c_up).  The ray from S down to the backwall and up to F has f(u) = h1 u / a_d + h2 u / a_u - X = 0 (h1 = zb - s,
// h2 = zb - zf, X = xf - x): f is odd, increasing and infinite at +-umax = +-min(1, kap), so the root is unique for h1, h2 > 0.
// Safeguarded Newton from u0 (bisection of the bracket when a step leaves it) until the step is below 1e-15; the last step is taken.
__host__ __device__ __forceinline__ double skip_inner(double h1, double h2, double X, double kap2, double umax, double u0, double& fu_out)
{
    double lo = -umax, hi = umax, u = u0, fu = NAN;
    for (int it = 0; it < 80; ++it) {
        const double ad2 = fma(-u, u, 1.0), au2 = fma(-u, u, kap2);
        const double rd = 1.0 / sqrt(ad2), ru = 1.0 / sqrt(au2);
        const double f = fma(u, fma(h1, rd, h2 * ru), -X);
        fu = fma(h1, rd * rd * rd, h2 * kap2 * (ru * ru * ru));
        if (f < 0.0) lo = u; else if (f > 0.0) hi = u; else break;
        const double step = -f / fu;
        const bool done = fabs(step) <= 1e-15 || !(hi - lo > 1e-15);
        // (a converged step that rounds onto u — now a bracket end — is kept: a bisection there would jump away from the root)
        double un = u + step;
        if (!(un >= lo && un <= hi)) un = done ? u : 0.5 * (lo + hi);
        u = un;
        if (done) break;
    }
    fu_out = fu;
    return u;
}

// the straight line from S to the mirrored point F' = (xf, 2 zb - zf), as a start for skip_inner
__host__ __device__ __forceinline__ double skip_u0(double h1, double h2, double X, double umax)
{
    const double h = h1 + h2;
    return umax * X / sqrt(fma(X, X, h * h));
}

// T, T', T'' of a skip leg: the element's leg as in surf_T, then T_in = (u X + h1 a_d + h2 a_u) / c_down with u solved in fp64;
// T_in' = -(u + a_d s') / c_down (envelope theorem), T_in'' = (1 - s' u / a_d)^2 / (c_down f_u) - a_d s'' / c_down (implicit
// differentiation of f = 0).  uw: the previous call's root (warm start), NaN for none; it is updated.
__device__ __forceinline__ Tder surf_T_skip(const double* __restrict__ coef, int n_s, double x0, double dx, double inv_dx, double inv_c1,
                                            double inv_cd, double kap2, double umax, double zb, double xe, double ze, double xf, double zf,
                                            double x, double& uw)
{
    double s, s1, s2;
    spline_eval(coef, n_s, x0, dx, inv_dx, x, s, s1, s2);
    const double ux = x - xe, uz = s - ze;
    const double q1 = fma(ux, ux, uz * uz);
    const double r1 = 1.0 / sqrt(q1);
    const double l1 = q1 * r1;
    const double A1 = fma(uz, s1, ux);
    const double B = fma(s1, s1, 1.0);
    const double h1 = zb - s, h2 = zb - zf, X = xf - x;
    double fu;
    const double u = skip_inner(h1, h2, X, kap2, umax, isnan(uw) ? skip_u0(h1, h2, X, umax) : uw, fu);
    uw = u;
    const double ad = sqrt(fma(-u, u, 1.0)), au = sqrt(fma(-u, u, kap2));
    const double w = fma(-s1 * u, 1.0 / ad, 1.0);
    Tder o;
    o.t = fma(l1, inv_c1, fma(u, X, fma(h1, ad, h2 * au)) * inv_cd);
    o.d1 = fma(A1 * r1, inv_c1, -fma(ad, s1, u) * inv_cd);
    o.d2 = fma((fma(uz, s2, B) - A1 * A1 * r1 * r1) * r1, inv_c1, (w * w / fu - ad * s2) * inv_cd);
    return o;
}

// per-angle constants of a plane wave (fp64, from the angle alone: the same bits in every slot and call); false when the angle is
// not finite or |angle| >= pi / 2
struct PwAngle { double sn, cs, tn, xref; bool ok; };
__device__ __forceinline__ PwAngle pw_angle(double th, double xlo, double xhi)
{
    PwAngle p;
    p.ok = fabs(th) < RTUS_PI_2;                                     // (NaN fails)
    const double t = p.ok ? th : 0.0;
    sincos(t, &p.sn, &p.cs);
    p.tn = p.sn / p.cs;
    p.xref = p.sn >= 0.0 ? xlo : xhi;
    return p;
}

// the least refined time over the kept brackets of one (element, focal point); written to tt (and xent).  T(x): the travel time
// and its derivatives at x; band(x): whether a root at x counts (always, for elements)
template <class TF, class BF>
__device__ __forceinline__ double surf_refine(TF T_at, BF band, int m, double x0, double hq, bool ok, float lb2, int j0, int j1, int j2,
                                              double* __restrict__ tt_out, double* __restrict__ xent_out)
{
    double best = NAN, bx = NAN;
    for (int k = 0; k < SURF_K; ++k) {
        const int j = k == 0 ? j0 : (k == 1 ? j1 : j2);
        // the third: not when the lower bound of its minimum's time (less the bound's fp32 error) is after the best refined time
        if (!ok || j < 0 || (k >= 2 && (double)lb2 > fma(4e-6, best, best))) continue;       // (best NaN: refined)
        int jl, jh;
        if (!rtus_bracket_fix(j, m, [&](int jp) { return T_at(fma((double)jp, hq, x0)).d1; }, jl, jh)) continue;
        double x;
        const Tder v = rtus_newton_min(T_at, fma((double)jl, hq, x0), fma((double)jh, hq, x0), 1e-10 * hq, x);
        if (!band(x)) continue;
        if (isnan(best) || v.t < best) { best = v.t; bx = x; }
    }
    *tt_out = best;
    if (xent_out) *xent_out = bx;
    return bx;
}

// the kernel's instantiations: element rows, plane-wave rows, element rows of a skip leg
enum SurfMode { SURF_ELEM = 0, SURF_PW = 1, SURF_SKIP = 2 };
#define SKIP_NEWTON 2       // fp32 Newton steps of the skip leg's inner slowness per (lane, scan point): scripts/skip_newton_study.py

template <int MODE>
__global__ void __launch_bounds__(RTUS_BLOCK) rtus_surface_kernel(SurfArgs a)
{
    __shared__ float4 sp[SURF_TILE];                                    // the tile's scan points
    __shared__ float4 sng[SURF_TILE][SURF_EB / 4];                      // -(c2 / c1) g1 per (point, element); PW: NaN out of band
                                                                        // (SKIP: c2 is c_down)
    __shared__ float4 st1[SURF_TILE][SURF_EB / 4];                      // |P - E| / c1 per (point, element); PW: the plane wave's time
    __shared__ float sxe[SURF_EB], sze[SURF_EB];
    // PW: per angle (fp32, scan coordinates): -(c2/c1) sin, -(c2/c1) cos, sin / c1, cos / c1, the time's offset, tan, band edges
    __shared__ float spw[8][SURF_EB];
    const int tid = threadIdx.x;
    const int f = blockIdx.x * RTUS_BLOCK + tid;
    const int e0 = blockIdx.y * SURF_EB;
    if (tid < SURF_EB) {
        const int e = e0 + tid < a.n_e ? e0 + tid : a.n_e - 1;
        if constexpr (MODE == SURF_PW) {
            const PwAngle w = pw_angle(a.ang[e], a.xlo, a.xhi);
            const double k21 = a.c2 / a.c1, nan = w.ok ? 0.0 : NAN;      // (an invalid angle: no bracket anywhere)
            spw[0][tid] = (float)(-k21 * w.sn + nan);
            spw[1][tid] = (float)(-k21 * w.cs + nan);
            spw[2][tid] = (float)(w.sn / a.c1);
            spw[3][tid] = (float)(w.cs / a.c1);
            spw[4][tid] = (float)(((a.xo - w.xref) * w.sn + (a.zo - a.za) * w.cs) / a.c1);
            spw[5][tid] = (float)w.tn;
            spw[6][tid] = (float)(a.xlo - a.xo);
            spw[7][tid] = (float)(a.xhi - a.xo);
            sze[tid] = (float)(a.za - a.zo);
        } else {
            sxe[tid] = (float)(a.xe[e] - a.xo);
            sze[tid] = (float)(a.ze[e] - a.zo);
        }
    }
    // the focal point: inside the extent and below the surface, else no path (NaN coordinates fail every test)
    double xf = 0.0, zf = 0.0;
    bool fok = false;
    if (f < a.n_f) {
        xf = a.xf[f];
        zf = a.zf[f];
        if (xf >= a.x0 && xf <= a.xend) {
            double s, s1, s2;
            spline_eval(a.coef, a.n_s, a.x0, a.dx, a.inv_dx, xf, s, s1, s2);
            fok = zf > s;
            if constexpr (MODE == SURF_SKIP) fok = fok && zf < a.zb;
        }
    }
    const float xfr = fok ? (float)(xf - a.xo) : NAN, zfr = fok ? (float)(zf - a.zo) : NAN;
    // SKIP: the lane's leg below the surface; u (= c_down p) is carried from scan point to scan point (fixed order: its bits depend
    // on the focal point and the profile alone), starting from the straight line to the mirrored point at the first one
    float h2f = 0.0f, uf = 0.0f;
    if constexpr (MODE == SURF_SKIP) {
        h2f = a.zbr - zfr;
        const float4 P = a.pts[0];
        const float X = xfr - P.x, h = (a.zbr - P.y) + h2f;
        uf = a.umaxf * X * __builtin_amdgcn_rsqf(fmaf(X, X, h * h));
    }

    float bt[SURF_EB][SURF_K];
    int bj[SURF_EB][SURF_K];
    bool neg[SURF_EB];
#pragma unroll
    for (int e = 0; e < SURF_EB; ++e) {
        neg[e] = false;
#pragma unroll
        for (int k = 0; k < SURF_K; ++k) { bt[e][k] = INFINITY; bj[e][k] = -1; }
    }
    for (int base = 0; base < a.m; base += SURF_TILE) {
        const int n = a.m - base < SURF_TILE ? a.m - base : SURF_TILE;
        __syncthreads();
        for (int i = tid; i < SURF_TILE * SURF_EB; i += RTUS_BLOCK) {
            const int j = i / SURF_EB, e = i % SURF_EB;
            const float4 P = j < n ? a.pts[base + j] : make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (MODE == SURF_PW) {
                // insonified: the point traced back along the incident direction lands on the aperture
                const float xb = fmaf(-(P.y - sze[e]), spw[5][e], P.x);
                const bool in = xb >= spw[6][e] && xb <= spw[7][e];
                ((float*)&sng[j][0])[e] = in ? fmaf(P.z, spw[1][e], spw[0][e]) : NAN;
                ((float*)&st1[j][0])[e] = fmaf(P.x, spw[2][e], fmaf(P.y, spw[3][e], spw[4][e]));
            } else {
                const float ux = P.x - sxe[e], uz = P.y - sze[e];
                const float q = fmaf(uz, uz, ux * ux);
                const float r = __builtin_amdgcn_rsqf(q);
                ((float*)&sng[j][0])[e] = -(fmaf(uz, P.z, ux) * r) * a.k21f;
                ((float*)&st1[j][0])[e] = q * r * a.ic1f;
            }
            if (e == 0) sp[j] = P;
        }
        __syncthreads();
        for (int jj = 0; jj < n; ++jj) {
            const float4 P = sp[jj];
            float g2, tin;                                              // T' c2 = g2 - ng: T' > 0 <=> g2 > ng; the leg's time
            if constexpr (MODE == SURF_SKIP) {
                // f(u) = h1 u / a_d + h2 u / a_u - X = 0; T_in c_down = u X + h1 a_d + h2 a_u, T_in' c_down = -(u + a_d s')
                const float h1 = a.zbr - P.y, X = xfr - P.x;
#pragma unroll
                for (int it = 0; it < SKIP_NEWTON; ++it) {
                    const float rd = __builtin_amdgcn_rsqf(fmaf(-uf, uf, 1.0f)), ru = __builtin_amdgcn_rsqf(fmaf(-uf, uf, a.kap2f));
                    const float fv = fmaf(uf, fmaf(h1, rd, h2f * ru), -X);
                    const float fu = fmaf(h1 * rd, rd * rd, h2f * a.kap2f * (ru * ru * ru));
                    const float un = fmaf(-fv, __builtin_amdgcn_rcpf(fu), uf);
                    uf = fabsf(un) < a.umaxf ? un : 0.5f * (uf + (fv < 0.0f ? a.umaxf : -a.umaxf));   // (NaN: toward an end)
                }
                const float ad2 = fmaf(-uf, uf, 1.0f), au2 = fmaf(-uf, uf, a.kap2f);
                const float ad = ad2 * __builtin_amdgcn_rsqf(ad2), au = au2 * __builtin_amdgcn_rsqf(au2);
                g2 = -fmaf(ad, P.z, uf);
                tin = fmaf(uf, X, fmaf(h1, ad, h2f * au));
            } else {
                const float vx = P.x - xfr, vz = P.y - zfr;
                const float q = fmaf(vz, vz, vx * vx);
                const float r = __builtin_amdgcn_rsqf(q);
                g2 = fmaf(vz, P.z, vx) * r;
                tin = q * r;
            }
            const float4 ng0 = sng[jj][0], ng1 = sng[jj][1];
            const float ng[SURF_EB] = {ng0.x, ng0.y, ng0.z, ng0.w, ng1.x, ng1.y, ng1.z, ng1.w};
            const int j = base + jj;
#pragma unroll
            for (int e = 0; e < SURF_EB; ++e) {
                const bool pos = g2 > ng[e];
                if (pos && neg[e]) {                                    // - -> + between P_j-1 and P_j: a minimum
                    // T(P_j) - hq T'(P_j): a lower bound of the minimum's time (T' c2 = g2 - ng)
                    const float t = fmaf(ng[e] - g2, a.hqic2f, fmaf(tin, a.ic2f, ((const float*)&st1[jj][0])[e]));
                    RTUS_KEEP3(t, j - 1, bt[e], bj[e]);
                }
                if constexpr (MODE == SURF_PW) neg[e] = !pos && ng[e] == ng[e];       // out of band (NaN): neither side of a bracket
                else neg[e] = !pos;                                     // (T' = 0 counts as -; NaN: never +)
            }
        }
    }
    if (f >= a.n_f) return;
    const double smin = a.smin[0], smax = MODE == SURF_SKIP ? a.smin[1] : 0.0;
    const double inv_c1 = 1.0 / a.c1, inv_c2 = 1.0 / a.c2;
#pragma unroll
    for (int e = 0; e < SURF_EB; ++e) {
        const int row = e0 + e;
        if (row < a.n_e) {
            const size_t o = (size_t)row * a.n_f + f;
            // the mode's T(x), which roots count and whether the row has paths at all (PW: the aperture's depth in ze's place)
            const PwAngle w = MODE == SURF_PW ? pw_angle(a.ang[row], a.xlo, a.xhi) : PwAngle{};
            const double xe = MODE == SURF_PW ? 0.0 : a.xe[row], ze = MODE == SURF_PW ? a.za : a.ze[row], kap2 = a.kap * a.kap;
            double uw = NAN;                                            // the skip leg's warm start, carried from call to call
            auto T_at = [&](double x) {
                if constexpr (MODE == SURF_PW)
                    return surf_T_pw(a.coef, a.n_s, a.x0, a.dx, a.inv_dx, inv_c1, inv_c2, w.sn, w.cs, w.xref, ze, xf, zf, x);
                else if constexpr (MODE == SURF_SKIP)
                    return surf_T_skip(a.coef, a.n_s, a.x0, a.dx, a.inv_dx, inv_c1, inv_c2, kap2, a.umax, a.zb, xe, ze, xf, zf, x, uw);
                else
                    return surf_T(a.coef, a.n_s, a.x0, a.dx, a.inv_dx, inv_c1, inv_c2, xe, ze, xf, zf, x);
            };
            auto band = [&](double x) {
                if constexpr (MODE == SURF_PW) {
                    double s, s1, s2;
                    spline_eval(a.coef, a.n_s, a.x0, a.dx, a.inv_dx, x, s, s1, s2);
                    const double xb = fma(-(s - ze), w.tn, x);
                    return xb >= a.xlo && xb <= a.xhi;
                }
                return true;
            };
            const bool ok = fok && ze < smin && (MODE != SURF_PW || w.ok) && (MODE != SURF_SKIP || a.zb > smax);
            const double bx = surf_refine(T_at, band, a.m, a.x0, a.hq, ok, bt[e][2], bj[e][0], bj[e][1], bj[e][2], a.tt + o,
                                          a.xent ? a.xent + o : nullptr);
            if (MODE == SURF_SKIP && a.xback) {                         // the reflection point of the winning root
                double xb = NAN;
                if (!isnan(bx)) {
                    double s, s1, s2, fu;
                    spline_eval(a.coef, a.n_s, a.x0, a.dx, a.inv_dx, bx, s, s1, s2);
                    const double h1 = a.zb - s, h2 = a.zb - zf, X = xf - bx;
                    const double u = skip_inner(h1, h2, X, kap2, a.umax, skip_u0(h1, h2, X, a.umax), fu);
                    xb = fma(h1, u / sqrt(fma(-u, u, 1.0)), bx);
                }
                a.xback[o] = xb;
            }
        }
    }
}

// the origin of the fp32 scan coordinates: the extent's centre; depths stay absolute (zs is device memory, and a few cm of depth
// is ~4e-9 m in fp32)
static double surf_xo(double x0, double dx, int n_s) { return x0 + 0.5 * (double)(n_s - 1) * dx; }
static const double surf_zo = 0.0;

// what every mode's table launch passes: the profile, the speeds (c2: below the surface), the rows' count, the grid, the workspace
static SurfArgs surf_args(double x0, double dx, int n_s, double c1, double c2, int n_rows, const double* xf, const double* zf, int n_f,
                          double* tt, double* xent, const SurfWs& w)
{
    SurfArgs a = {};
    a.x0 = x0; a.dx = dx; a.hq = dx / SURF_SUB; a.inv_dx = 1.0 / dx; a.xend = fma((double)(n_s - 1), dx, x0);
    a.c1 = c1; a.c2 = c2;
    a.xo = surf_xo(x0, dx, n_s); a.zo = surf_zo;
    a.ic1f = (float)(1.0 / c1); a.ic2f = (float)(1.0 / c2); a.k21f = (float)(c2 / c1); a.hqic2f = (float)(a.hq / c2);
    a.n_s = n_s; a.m = surf_points(n_s); a.n_e = n_rows; a.n_f = n_f;
    a.xf = xf; a.zf = zf; a.tt = tt; a.xent = xent;
    a.coef = w.coef; a.pts = w.pts; a.smin = w.smin;
    return a;
}

// the set-up kernel, then the table kernel of one mode
template <int MODE>
static hipError_t surf_launch(const SurfArgs& a, const double* zs, const SurfWs& w, hipStream_t s)
{
    const long long gy = ((long long)a.n_e + SURF_EB - 1) / SURF_EB, gx = ((long long)a.n_f + RTUS_BLOCK - 1) / RTUS_BLOCK;
    if (gy > 65535 || gx > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rtus_surface_setup_kernel, dim3(1), dim3(RTUS_BLOCK), 0, s, zs, a.n_s, a.x0, a.dx, a.xo, a.zo, w);
    hipLaunchKernelGGL(rtus_surface_kernel<MODE>, dim3((unsigned)gx, (unsigned)gy), dim3(RTUS_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t rtus_launch_tt_surface(double x0, double dx, const double* zs, int n_s, double c1, double c2, const double* xe,
                                  const double* ze, int n_e, const double* xf, const double* zf, int n_f, double* tt, double* xent,
                                  void* ws, hipStream_t s)
{
    const SurfWs w = surf_ws(ws, n_s);
    SurfArgs a = surf_args(x0, dx, n_s, c1, c2, n_e, xf, zf, n_f, tt, xent, w);
    a.xe = xe; a.ze = ze;
    return surf_launch<SURF_ELEM>(a, zs, w, s);
}

// plane waves: angles in the elements' place (the set-up kernel and its workspace as above)
hipError_t rtus_launch_pw_surface(double x0, double dx, const double* zs, int n_s, double c1, double c2, const double* ang, int n_a,
                                  double xlo, double xhi, double za, const double* xf, const double* zf, int n_f, double* tt, double* xent,
                                  void* ws, hipStream_t s)
{
    const SurfWs w = surf_ws(ws, n_s);
    SurfArgs a = surf_args(x0, dx, n_s, c1, c2, n_a, xf, zf, n_f, tt, xent, w);
    a.ang = ang; a.xlo = xlo; a.xhi = xhi; a.za = za;
    return surf_launch<SURF_PW>(a, zs, w, s);
}

// skip legs: elements, the leg below the surface down in c_down to the backwall at z_back and up in c_up to the point
hipError_t rtus_launch_tt_surface_skip(double x0, double dx, const double* zs, int n_s, double c1, double c_down, double c_up, double z_back,
                                       const double* xe, const double* ze, int n_e, const double* xf, const double* zf, int n_f, double* tt,
                                       double* xent, double* xback, void* ws, hipStream_t s)
{
    const SurfWs w = surf_ws(ws, n_s);
    SurfArgs a = surf_args(x0, dx, n_s, c1, c_down, n_e, xf, zf, n_f, tt, xent, w);
    a.xe = xe; a.ze = ze;
    a.zb = z_back; a.kap = c_down / c_up; a.umax = a.kap < 1.0 ? a.kap : 1.0;
    a.zbr = (float)(z_back - a.zo); a.kap2f = (float)(a.kap * a.kap);
    a.umaxf = (float)a.umax * (1.0f - 1e-6f);                 // (the fp32 scan stays off the ends, where a_d or a_u is 0)
    a.xback = xback;
    return surf_launch<SURF_SKIP>(a, zs, w, s);
}

// the set-up kernel alone (rtus_spline.h)
hipError_t rtus_launch_surface_setup(const double* zs, int n_s, double x0, double dx, void* ws, const double** coef, hipStream_t s)
{
    const SurfWs w = surf_ws(ws, n_s);
    *coef = w.coef;
    hipLaunchKernelGGL(rtus_surface_setup_kernel, dim3(1), dim3(RTUS_BLOCK), 0, s, zs, n_s, x0, dx, surf_xo(x0, dx, n_s), surf_zo, w);
    return hipGetLastError();
}

// ... and where it leaves the scan points and the depth extremes (rtus_spline.h)
hipError_t rtus_launch_surface_setup_scan(const double* zs, int n_s, double x0, double dx, void* ws, RtusSurfaceScan* scan, hipStream_t s)
{
    const SurfWs w = surf_ws(ws, n_s);
    *scan = RtusSurfaceScan{w.coef, w.pts, w.smin, surf_xo(x0, dx, n_s), surf_zo, surf_points(n_s)};
    hipLaunchKernelGGL(rtus_surface_setup_kernel, dim3(1), dim3(RTUS_BLOCK), 0, s, zs, n_s, x0, dx, scan->xo, scan->zo, w);
    return hipGetLastError();
}
