// rtus_lens_pipe.hip — element x focal-point Fermat travel times from the elements behind the reference's curved lens, through
// the water, into the WALL of the pipe: two curved refractions (the lens surface P(alpha), then the pipe's outer circle Q(beta)).
// NOT IN THE REFERENCE (it defines the wall speed c3 = 5600 and never uses it); checked against tests/pipe_numpy.py, itself checked
// against a 40-digit joint solve in (alpha, beta) (tests/test_pipe_cpu.py).
//
//   T(beta)       = T_lens(E, Q(beta)) + |Q(beta) - F| / c3,   Q(beta) = (x_off + r_outer sin beta, r_outer cos beta)
//   T_lens(E, Q)  = the least time over alpha in [a_lo, a_hi] of the lens leg (rtus_tt_lens's entry for the target Q)
//   entry         = the least T over the interior local minima of T on (b_lo, b_hi) whose path qualifies (include/rtus.h)
//
//   1. rtus_pipe_setup_kernel: one lane per (element, scan point beta_j = b_lo + j hb): the lens leg to Q_j solved on its own —
//      rtus_tt_lens's generic step (T, g at PIPE_NS + 1 even samples of alpha, the zero of g in every cell that brackets a
//      minimum by safeguarded Newton, least T wins, the ends included), never a continuation from a neighbouring lane: the bits
//      depend on (element, beta_j) alone.  Into the workspace: alpha*, the fp32 time and -(c3 / c2) u . Q' (u the unit water
//      direction at Q_j: c2 dT_lens / dbeta by the envelope theorem); the scan points (Q_j - Cp, Q'_j) as fp32.
//   2. rtus_pipe_kernel: the bracket scan of rtus_bracket.h.  Lanes are focal points, a workgroup owns PIPE_EB elements, scan points are
//      tiled through LDS with the element terms as broadcasts; the lane's term v . Q' (v = (Q - F) / |Q - F|) is shared by the
//      workgroup's elements.  A sign change - -> + of dT/dbeta is a bracket, ranked by an fp32 estimate of T; PIPE_K are kept.
//   3. Each kept bracket is refined in fp64 (rtus_bracket.h): the fp64 bracket, then safeguarded Newton in beta.
//      Every iterate solves the inner alpha to convergence (lens_time<double, true>), warm-started from the table's alpha at the
//      bracket's end and then from the previous iterate; a suspect inner minimum (g' < gp_min or pinned at an end: rtus_tt_lens's
//      own test) takes the whole interval's least time instead (the set-up kernel's step).  T'' by implicit differentiation:
//      T_lens'' = [(|Q'|^2 - (u.Q')^2) / l + u.Q''] / c2 - (g_aQ . Q')^2 / g' (the last term only at an interior inner minimum).
//      The refined path qualifies when its water segment arrives from outside the circle and its wall segment keeps off the bore.
//
// Determinism: an entry is made from its element, its focal point and the parameters only (the table entries it reads are
// functions of (element, beta_j)); not of its slot, its lane or whatever else shares the call.
//
// The SKIP leg (rtus_tt_pipe_skip: Q -> a bounce off the bore at R(gamma) -> F, c_down before and c_up after it) is the same scan
// and refine with the wall leg |Q - F| / c3 replaced by W(Q, F) = min over gamma of |Q - R| / c_down + |R - F| / c_up, an inner
// solve that belongs to (beta, F) alone.  In the angles u = gamma - beta, v = gamma - theta_F (theta_F, r_F: F about the centre):
//   |Q - R|^2 = (ro - ri)^2 + 4 ro ri sin^2(u / 2),  |R - F|^2 = (r_F - ri)^2 + 4 r_F ri sin^2(v / 2)
//   h = dW_path / dgamma = A(u) + B(v),  A = ro ri sin u / (|Q - R| c_down),  B = r_F ri sin v / (|R - F| c_up)
//   A' = ro ri (ro cos u - ri)(ro - ri cos u) / (|Q - R|^3 c_down) > 0 exactly where Q sees R (and B' likewise for F): on the arc
//   that both see the path's time is convex, so W exists iff h < 0 at the arc's lower end and h > 0 at its upper end, the
//   minimum is unique, and it lies between beta and theta_F (where the two sines have opposite signs).
//   dW/dbeta = -A (envelope theorem), d2W/dbeta2 = A' B' / (A' + B') (implicit differentiation of h = 0).
// The scan solves u in fp32 per (scan point, lane) by safeguarded Newton, warm-started in v from the previous scan point (a
// function of (F, j) only); a beta without W is neither side of a bracket.  The refine solves it in fp64 at every iterate, beside
// the inner alpha: two independent inner solves.  Only rule 1 applies (the wall segments keep off the bore by construction).
#include <type_traits>
#include "rtus_lens.h"
#include "rtus_bracket.h"

#define PIPE_EB 8           // elements per workgroup
#define PIPE_TILE 64        // scan points per LDS tile
#define PIPE_K 3            // brackets kept per (element, focal point)
#define PIPE_NS 32          // even samples of alpha in a whole-interval solve of the lens leg

struct PipeArgs {
    LensConst<double> k;               // lens constants (lens_time's)
    double a_lo, a_hi, gp_min;         // alpha interval; g' below gp_min: the inner minimum is suspect
    double r_out, r_in, x_off, ic3;    // the pipe; 1 / c3
    double b_lo, hb;                   // scan points beta_j = b_lo + j hb, j < m
    float k32f, ic3f;                  // c3 / c2, 1 / c3
    int m, n_e, n_f;
    const double* __restrict__ xe;
    const double* __restrict__ ze;
    const double* __restrict__ xf;
    const double* __restrict__ zf;
    double* __restrict__ tt;
    double* __restrict__ alpha_out;    // nullable
    double* __restrict__ beta_out;     // nullable
    float4* __restrict__ pts;          // [m]: (Q - Cp, Q') fp32
    float2* __restrict__ ent;          // [n_e][m]: (-(c3 / c2) u . Q', T_lens) fp32
    double* __restrict__ al;           // [n_e][m]: alpha* fp64
};

// workspace: pts [m] | ent [n_e][m] | al [n_e][m], 256-byte aligned pieces; returns its size (a: the pieces' pointers, nullable)
static size_t pipe_ws(void* ws, int n_e, int m, PipeArgs* a)
{
    const size_t nm = (size_t)n_e * (size_t)m;
    const size_t o_ent = rtus_al256(16 * (size_t)m), o_al = o_ent + rtus_al256(8 * nm);
    if (a) {
        a->pts = (float4*)ws;
        a->ent = (float2*)((char*)ws + o_ent);
        a->al = (double*)((char*)ws + o_al);
    }
    return o_al + rtus_al256(8 * nm);
}
size_t rtus_pipe_ws_bytes(int n_e, int m) { return pipe_ws(nullptr, n_e, m, nullptr); }

// The lens leg's least time over the whole interval (rtus_tt_lens's generic step, per lane): T and g at PIPE_NS + 1 even samples
// (any sample bounds the least time from above: a minimum pinned at an end comes in here), and in every cell whose ends say "a
// minimum inside" (g < 0 left, g >= 0 right) the zero of g by safeguarded Newton.  Returns alpha; T is its time.
template <bool POLY>
__device__ double lens_leg_min(const LensConst<double>& k, double a_lo, double a_hi, double xa, double za, double qx, double qz, double& T)
{
    const double dA = (a_hi - a_lo) * (1.0 / PIPE_NS);
    double bA = a_lo, bT, pg, gp;
    lens_time<double, false, POLY>(k, a_lo, xa, za, qx, qz, bT, pg, gp);
    double pa = a_lo;
    for (int j = 1; j <= PIPE_NS; ++j) {
        const double ca = j == PIPE_NS ? a_hi : fma((double)j, dA, a_lo);
        double cT, cg;
        lens_time<double, false, POLY>(k, ca, xa, za, qx, qz, cT, cg, gp);
        if (cT < bT) { bT = cT; bA = ca; }
        if (pg < 0.0 && cg >= 0.0) {
            // (only the converged point competes: near the focus T is flat enough in alpha for an iterate 1e-8 rad off to be
            // "earlier" by rounding, and dT/dbeta at the wrong alpha is off by far more than the time is)
            double lo = pa, hi = ca, x = 0.5 * (pa + ca);
            for (int it = 0; it < 60; ++it) {
                double t, g;
                lens_time<double, true, POLY>(k, x, xa, za, qx, qz, t, g, gp);
                if (g < 0.0) lo = x; else hi = x;
                const double step = -g / gp;
                double xn = x + step;
                const bool done = (gp > 0.0 && fabs(step) <= 1e-13) || !(hi - lo > 1e-13);
                if (!(gp > 0.0) || !(xn > lo && xn < hi)) xn = done ? x : 0.5 * (lo + hi);
                x = xn;
                if (done) break;
            }
            double t, g;
            lens_time<double, false, POLY>(k, x, xa, za, qx, qz, t, g, gp);
            if (t < bT) { bT = t; bA = x; }
        }
        pa = ca; pg = cg;
    }
    T = bT;
    return bA;
}

__device__ __forceinline__ void pipe_q(const PipeArgs& a, double beta, double& qx, double& qz, double& q1x, double& q1z)
{
    double s, c;
    sincos(beta, &s, &c);
    qx = fma(a.r_out, s, a.x_off); qz = a.r_out * c;
    q1x = a.r_out * c; q1z = -a.r_out * s;
}

// ---- the skip leg's inner solve
struct PipeSkip {
    double icu, aQ, dQ;                // 1 / c_up; arccos(ri / ro): half the arc of the bore that Q sees; ro - ri
    float icuf, aQf, dQf;
    double* __restrict__ gamma_out;    // nullable
};
struct BoreW { double w, d1, d2, gamma, v; };    // W, dW/dbeta, d2W/dbeta2, the bounce's angle, v; NaN without W
struct BoreK { double ro, ri, icd, icu, aQ, dQ, rF, thF, aF, dF; };      // bore_W's constants, passed by value (registers)

#define RTUS_TWO_PI 6.283185307179586476925286766559
// the arc's ends in u and the root's bracket inside it (lo1, hi1): false when the arc is empty or the root lies outside it
template <class R>
__device__ __forceinline__ bool bore_arc(R aQ, R aF, R dl, R& lo0, R& hi0, R& lo1, R& hi1)
{
    lo0 = aQ * R(-1) > dl - aF ? aQ * R(-1) : dl - aF;
    hi0 = aQ < dl + aF ? aQ : dl + aF;
    const R z0 = dl < R(0) ? dl : R(0), z1 = dl > R(0) ? dl : R(0);
    lo1 = lo0 > z0 ? lo0 : z0;
    hi1 = hi0 < z1 ? hi0 : z1;
    return hi0 > lo0 && hi1 >= lo1;
}

// h = A icd + B icu and h' at u (Ag, Bg, Ap, Bp: the terms without / with the speeds), W the path's time
__device__ __forceinline__ void bore_h(const BoreK& c, double u, double dl, double& h, double& Ag, double& Ap, double& Bp, double& W)
{
    double s2, c2, t2, e2;
    sincos(0.5 * u, &s2, &c2);
    sincos(0.5 * (u - dl), &t2, &e2);
    const double su = 2.0 * s2 * c2, cu = fma(-2.0 * s2, s2, 1.0), sv = 2.0 * t2 * e2, cv = fma(-2.0 * t2, t2, 1.0);
    const double rr = c.ro * c.ri, fr = c.rF * c.ri;
    const double lq2 = fma(4.0 * rr * s2, s2, c.dQ * c.dQ), lf2 = fma(4.0 * fr * t2, t2, c.dF * c.dF);
    const double lq = sqrt(lq2), lf = sqrt(lf2);
    Ag = rr * su / lq;
    Ap = rr * (fma(c.ro, cu, -c.ri) * fma(-c.ri, cu, c.ro)) / (lq2 * lq) * c.icd;
    Bp = fr * (fma(c.rF, cv, -c.ri) * fma(-c.ri, cv, c.rF)) / (lf2 * lf) * c.icu;
    h = fma(Ag, c.icd, fr * sv / lf * c.icu);
    W = fma(lq, c.icd, lf * c.icu);
}

// W(Q(beta), F) in fp64: safeguarded Newton on h from the warm start vw (v of the previous call; NaN: from the end of the root's
// bracket nearer to theta_F), bracket kept by the sign of h.  Everything by value (a pointer to a lane's local would put it in
// scratch) and left to the inliner: marked noinline the call frame costs 104 B of scratch, inlined the kernel has none.
__device__ BoreW bore_W(BoreK c, double v0, double beta)
{
    BoreW o;
    o.w = o.d1 = o.d2 = o.gamma = o.v = NAN;
    double dl = c.thF - beta;
    dl = fma(-RTUS_TWO_PI, rint(dl * (1.0 / RTUS_TWO_PI)), dl);
    double lo0, hi0, lo, hi, h, Ag, Ap, Bp, W;
    if (!bore_arc<double>(c.aQ, c.aF, dl, lo0, hi0, lo, hi)) return o;
    if (lo == lo0) { bore_h(c, lo0, dl, h, Ag, Ap, Bp, W); if (!(h < 0.0)) return o; }
    if (hi == hi0) { bore_h(c, hi0, dl, h, Ag, Ap, Bp, W); if (!(h > 0.0)) return o; }
    double u = v0 + dl;
    if (!(u >= lo && u <= hi)) u = fmin(fmax(dl, lo), hi);
    for (int it = 0; it < 80; ++it) {
        bore_h(c, u, dl, h, Ag, Ap, Bp, W);
        if (h == 0.0) break;
        if (h < 0.0) lo = u; else hi = u;
        const double step = -h / (Ap + Bp);
        double un = u + step;
        const bool done = fabs(step) <= 1e-14 || !(hi - lo > 1e-14);
        if (!(un >= lo && un <= hi)) un = done ? u : 0.5 * (lo + hi);
        u = un;
        if (done) { bore_h(c, u, dl, h, Ag, Ap, Bp, W); break; }
    }
    o.w = W;
    o.d1 = -Ag * c.icd;
    o.d2 = Ap * Bp / (Ap + Bp);
    o.gamma = beta + u;
    o.v = u - dl;
    return o;
}

// the scan's fp32 evaluation: h, h', Ag and W at u
__device__ __forceinline__ void bore_h32(float rr, float fr, float ro, float ri, float rF, float dQ, float dF, float icd, float icu, float u,
                                         float dl, float& h, float& hp, float& Ag, float& W)
{
    const float hu = 0.5f * u, hv = 0.5f * (u - dl);
    const float s2 = __sinf(hu), c2 = __cosf(hu), t2 = __sinf(hv), e2 = __cosf(hv);
    const float su = 2.0f * s2 * c2, cu = fmaf(-2.0f * s2, s2, 1.0f), sv = 2.0f * t2 * e2, cv = fmaf(-2.0f * t2, t2, 1.0f);
    const float lq2 = fmaf(4.0f * rr * s2, s2, dQ * dQ), lf2 = fmaf(4.0f * fr * t2, t2, dF * dF);
    const float iq = __builtin_amdgcn_rsqf(lq2), jf = __builtin_amdgcn_rsqf(lf2);
    Ag = rr * su * iq;
    h = fmaf(Ag, icd, fr * sv * jf * icu);
    hp = fmaf(rr * (fmaf(ro, cu, -ri) * fmaf(-ri, cu, ro)) * (iq * iq * iq), icd,
              fr * (fmaf(rF, cv, -ri) * fmaf(-ri, cv, rF)) * (jf * jf * jf) * icu);
    W = fmaf(lq2 * iq, icd, lf2 * jf * icu);
}

template <bool POLY>
__global__ void __launch_bounds__(RTUS_BLOCK) rtus_pipe_setup_kernel(PipeArgs a)
{
    const long long t = (long long)blockIdx.x * RTUS_BLOCK + threadIdx.x;
    if (t >= (long long)a.n_e * a.m) return;
    const int e = (int)(t / a.m), j = (int)(t - (long long)e * a.m);
    const double beta = fma((double)j, a.hb, a.b_lo);
    double qx, qz, q1x, q1z;
    pipe_q(a, beta, qx, qz, q1x, q1z);
    if (e == 0) a.pts[j] = make_float4((float)(qx - a.x_off), (float)qz, (float)q1x, (float)q1z);
    const double xa = a.xe[e], za = a.ze[e];
    double T = NAN, alpha = NAN;
    float ng = NAN;
    if (isfinite(xa) && isfinite(za)) {
        alpha = lens_leg_min<POLY>(a.k, a.a_lo, a.a_hi, xa, za, qx, qz, T);
        double px, pz, p1x, p1z;
        lens_point<POLY>(a.k, alpha, px, pz, p1x, p1z);
        const double ux = qx - px, uz = qz - pz, r = 1.0 / sqrt(fma(ux, ux, uz * uz));
        ng = (float)(-(double)a.k32f * (fma(ux, q1x, uz * q1z) * r));
    }
    a.ent[t] = make_float2(ng, (float)T);
    a.al[t] = alpha;
}

// T(beta) and its first two derivatives for one (element, focal point), with the path's lens point and the inner alpha
struct PipeT { double t, d1, d2, alpha, px, pz, qx, qz; };
struct PipeTS : PipeT { double gamma, v; };

// S...: nothing for the direct leg; (BoreK, double v0) for the skip leg: bore_W's constants and the inner gamma's warm start, by value
template <bool POLY, class... S>
__device__ std::conditional_t<(sizeof...(S) > 0), PipeTS, PipeT> pipe_T(const PipeArgs& a, double xa, double za, double xf, double zf,
                                                                       double beta, double& aw, S... skip)
{
    constexpr bool SKIP = sizeof...(S) > 0;
    const LensConst<double>& k = a.k;
    double qx, qz, q1x, q1z;
    pipe_q(a, beta, qx, qz, q1x, q1z);
    // inner: safeguarded Newton on g = dT_lens / dalpha from the warm start, bracket kept by the sign of g
    double alpha = fmin(fmax(aw, a.a_lo), a.a_hi), lo = a.a_lo, hi = a.a_hi, T = NAN, g = NAN, gp = NAN;
    for (int it = 0; it < 80; ++it) {
        lens_time<double, true, POLY>(k, alpha, xa, za, qx, qz, T, g, gp);
        if (g > 0.0) hi = alpha; else lo = alpha;
        const double step = -g / gp;
        double next = alpha + step;
        const bool done = (gp > 0.0 && fabs(step) <= 1e-13) || !(hi - lo > 1e-13);
        if (!(gp > 0.0) || !(next >= lo && next <= hi)) next = done ? alpha : 0.5 * (lo + hi);
        alpha = next;
        if (done) break;
    }
    lens_time<double, true, POLY>(k, alpha, xa, za, qx, qz, T, g, gp);
    // a minimum beyond an end: the bisections stop within 1e-13 of it, the least time is AT the end (and suspect: below)
    if (g < 0.0 && a.a_hi - alpha <= 2e-13) alpha = a.a_hi;
    if (g > 0.0 && alpha - a.a_lo <= 2e-13) alpha = a.a_lo;
    bool interior = gp > 0.0 && alpha > a.a_lo && alpha < a.a_hi;
    if (!(interior && gp >= a.gp_min)) {                     // suspect: the whole interval's least time
        double Tm;
        const double am = lens_leg_min<POLY>(k, a.a_lo, a.a_hi, xa, za, qx, qz, Tm);
        if (am != alpha) {
            alpha = am;
            lens_time<double, true, POLY>(k, alpha, xa, za, qx, qz, T, g, gp);
        }
        interior = gp > 0.0 && alpha > a.a_lo && alpha < a.a_hi;
    }
    aw = alpha;
    double px, pz, p1x, p1z;
    lens_point<POLY>(k, alpha, px, pz, p1x, p1z);
    const double inv_c2 = k.c2inv;
    // lens leg: dT/dQ = u / c2 (envelope theorem)
    const double ux0 = qx - px, uz0 = qz - pz, l = sqrt(fma(ux0, ux0, uz0 * uz0)), il = 1.0 / l;
    const double ux = ux0 * il, uz = uz0 * il;
    const double q2x = -(qx - a.x_off), q2z = -qz;                     // Q''
    const double QQ = fma(q1x, q1x, q1z * q1z), uQ = fma(ux, q1x, uz * q1z), uP = fma(ux, p1x, uz * p1z);
    const double gaq = -(fma(p1x, q1x, p1z * q1z) - uP * uQ) * il * inv_c2;     // d g / dQ . Q'
    double d2l = (fma(-uQ, uQ, QQ) * il + fma(ux, q2x, uz * q2z)) * inv_c2;
    if (interior) d2l -= gaq * gaq / gp;
    std::conditional_t<SKIP, PipeTS, PipeT> o;
    if constexpr (SKIP) {
        // wall legs: down to the bore and up to F
        const BoreW w = bore_W(skip..., beta);
        o.t = T + w.w;
        o.d1 = fma(uQ, inv_c2, w.d1);
        o.d2 = d2l + w.d2;
        o.gamma = w.gamma;
        o.v = w.v;
    } else {
        // wall leg
        const double vx0 = qx - xf, vz0 = qz - zf, mq = sqrt(fma(vx0, vx0, vz0 * vz0)), im = 1.0 / mq;
        const double vx = vx0 * im, vz = vz0 * im, vQ = fma(vx, q1x, vz * q1z);
        o.t = fma(mq, a.ic3, T);
        o.d1 = fma(uQ, inv_c2, vQ * a.ic3);
        o.d2 = d2l + (fma(-vQ, vQ, QQ) * im + fma(vx, q2x, vz * q2z)) * a.ic3;
    }
    o.alpha = alpha; o.px = px; o.pz = pz; o.qx = qx; o.qz = qz;
    return o;
}

// the table kernel's body: the direct leg (SKIP false: k is not read) or the skip leg
template <bool POLY, bool SKIP>
__device__ __forceinline__ void pipe_table(const PipeArgs& a, const PipeSkip& k)
{
    __shared__ float4 sp[PIPE_TILE];                         // the tile's scan points (Q - Cp, Q')
    __shared__ float2 sen[PIPE_TILE][PIPE_EB];               // per (point, element): -(c3 / c2) u . Q', T_lens
    const int tid = threadIdx.x;
    const int f = blockIdx.x * RTUS_BLOCK + tid;
    const int e0 = blockIdx.y * PIPE_EB;
    // the focal point: strictly inside the wall, else no path (NaN coordinates fail every test of the scan)
    double xf = 0.0, zf = 0.0;
    bool fok = false;
    if (f < a.n_f) {
        xf = a.xf[f];
        zf = a.zf[f];
        const double dx = xf - a.x_off, rf = sqrt(fma(dx, dx, zf * zf));
        fok = rf > a.r_in && rf < a.r_out;
    }
    const float xfr = fok ? (float)(xf - a.x_off) : NAN, zfr = fok ? (float)zf : NAN;
    // skip leg: F about the centre, and the scan's fp32 copies
    BoreK L;                                                 // (rF, thF: F about the centre; aF = arccos(ri / rF); dF = rF - ri)
    float rrf = 0.f, frf = 0.f, rof = 0.f, rif = 0.f, rFf = 0.f, dFf = 0.f, aFf = 0.f, vwf = NAN;
    if constexpr (SKIP) {
        const double dx = xf - a.x_off;
        L.rF = sqrt(fma(dx, dx, zf * zf));
        L.thF = atan2(dx, zf);
        L.aF = acos(a.r_in / L.rF);
        L.dF = L.rF - a.r_in;
        L.ro = a.r_out; L.ri = a.r_in; L.icd = a.ic3; L.icu = k.icu; L.aQ = k.aQ; L.dQ = k.dQ;
        rrf = (float)(a.r_out * a.r_in); frf = (float)(L.rF * a.r_in);
        rof = (float)a.r_out; rif = (float)a.r_in; rFf = (float)L.rF; dFf = (float)L.dF; aFf = (float)L.aF;
    }

    float bt[PIPE_EB][PIPE_K];
    int bj[PIPE_EB][PIPE_K];
    bool neg[PIPE_EB];
#pragma unroll
    for (int e = 0; e < PIPE_EB; ++e) {
        neg[e] = false;
#pragma unroll
        for (int k = 0; k < PIPE_K; ++k) { bt[e][k] = INFINITY; bj[e][k] = -1; }
    }
    for (int base = 0; base < a.m; base += PIPE_TILE) {
        const int n = a.m - base < PIPE_TILE ? a.m - base : PIPE_TILE;
        __syncthreads();
        for (int i = tid; i < PIPE_TILE * PIPE_EB; i += RTUS_BLOCK) {
            const int j = i / PIPE_EB, e = i % PIPE_EB;
            const int row = e0 + e < a.n_e ? e0 + e : a.n_e - 1;
            sen[j][e] = j < n ? a.ent[(size_t)row * a.m + base + j] : make_float2(NAN, NAN);
            if (e == 0) sp[j] = j < n ? a.pts[base + j] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();
        for (int jj = 0; jj < n; ++jj) {
            float g, tw;
            if constexpr (SKIP) {
                // the bounce at beta_j: u by safeguarded Newton from the previous scan point's v; NaN without W
                g = NAN; tw = NAN;
                double dld = L.thF - fma((double)(base + jj), a.hb, a.b_lo);
                dld = fma(-RTUS_TWO_PI, rint(dld * (1.0 / RTUS_TWO_PI)), dld);
                const float dl = (float)dld;
                float lo0, hi0, lo, hi, h, hp, Ag, W;
                bool ok = bore_arc<float>(k.aQf, aFf, dl, lo0, hi0, lo, hi) && fok;
                if (ok && lo == lo0) { bore_h32(rrf, frf, rof, rif, rFf, k.dQf, dFf, a.ic3f, k.icuf, lo0, dl, h, hp, Ag, W); ok = h < 0.f; }
                if (ok && hi == hi0) { bore_h32(rrf, frf, rof, rif, rFf, k.dQf, dFf, a.ic3f, k.icuf, hi0, dl, h, hp, Ag, W); ok = h > 0.f; }
                float u = vwf + dl;
                vwf = NAN;
                if (ok) {
                    if (!(u >= lo && u <= hi)) u = fminf(fmaxf(dl, lo), hi);
                    for (int it = 0; it < 16; ++it) {
                        bore_h32(rrf, frf, rof, rif, rFf, k.dQf, dFf, a.ic3f, k.icuf, u, dl, h, hp, Ag, W);
                        if (h < 0.f) lo = u; else hi = u;
                        const float step = -h / hp;
                        float un = u + step;
                        const bool done = fabsf(step) <= 2e-7f || !(hi - lo > 2e-7f);
                        if (!(un >= lo && un <= hi)) un = done ? u : 0.5f * (lo + hi);
                        u = un;
                        if (done) break;
                    }
                    bore_h32(rrf, frf, rof, rif, rFf, k.dQf, dFf, a.ic3f, k.icuf, u, dl, h, hp, Ag, W);
                    g = -Ag;                                       // c_down dW / dbeta
                    tw = W;
                    vwf = u - dl;
                }
            } else {
                const float4 P = sp[jj];
                const float vx = P.x - xfr, vz = P.y - zfr;
                const float q = fmaf(vz, vz, vx * vx);
                const float r = __builtin_amdgcn_rsqf(q);
                g = fmaf(vz, P.w, vx * P.z) * r;                   // c3 dT_wall / dbeta
                tw = q * r * a.ic3f;
            }
            const int j = base + jj;
#pragma unroll
            for (int e = 0; e < PIPE_EB; ++e) {
                const float2 s = sen[jj][e];
                const bool pos = g > s.x;                          // dT / dbeta > 0 (NaN: never)
                if (pos && neg[e]) {                               // - -> + between beta_j-1 and beta_j: a minimum
                    const float t = s.y + tw;
                    RTUS_KEEP3(t, j - 1, bt[e], bj[e]);
                }
                neg[e] = !pos && s.x == s.x;                       // (an element without a lens leg: neither side of a bracket)
                if constexpr (SKIP) neg[e] = neg[e] && g == g;     // (nor is a beta without a bounce)
            }
        }
    }
    if (f >= a.n_f) return;
    const double rin2 = a.r_in * a.r_in;
#pragma unroll 1
    for (int e = 0; e < PIPE_EB; ++e) {
        const int row = e0 + e;
        if (row >= a.n_e) break;
        const size_t o = (size_t)row * a.n_f + f;
        const double xa = a.xe[row], za = a.ze[row];
        const double* alr = a.al + (size_t)row * a.m;
        // this element's brackets by selects over constant indices (an index by the loop's e would put the arrays in scratch)
        float et[PIPE_K];
        int ej[PIPE_K];
#pragma unroll
        for (int kk = 0; kk < PIPE_K; ++kk) {
            et[kk] = bt[0][kk]; ej[kk] = bj[0][kk];
#pragma unroll
            for (int q = 1; q < PIPE_EB; ++q) { et[kk] = q == e ? bt[q][kk] : et[kk]; ej[kk] = q == e ? bj[q][kk] : ej[kk]; }
        }
        // the third bracket is skipped only once an earlier one has given a qualifying time and the fp32 estimate puts the third
        // clearly (4e-6) after it; while the earlier ones were rejected by a rule it is refined however late it is
        float tb = INFINITY;                                       // fp32 time of the bracket that gave best
        double best = NAN, bA = NAN, bB = NAN, bG = NAN;
        for (int kk = 0; kk < PIPE_K; ++kk) {
            const int j = kk == 0 ? ej[0] : (kk == 1 ? ej[1] : ej[2]);
            const float tk = kk == 0 ? et[0] : (kk == 1 ? et[1] : et[2]);
            if (!fok || j < 0 || (kk >= 2 && !(tk <= fmaf(4e-6f, tb, tb)))) continue;
            // the fp64 bracket (beta_j-1 .. beta_j+2 at most); the inner alpha at a scan point starts from the table's alpha there
            int jl, jh;
            double vw = NAN;                                      // (skip leg: the inner gamma's warm start, from iterate to iterate)
            auto d1_at = [&](int jp) {
                double aw = alr[jp];
                if constexpr (SKIP)
                    return pipe_T<POLY>(a, xa, za, xf, zf, fma((double)jp, a.hb, a.b_lo), aw, L, (double)NAN).d1;
                else
                    return pipe_T<POLY>(a, xa, za, xf, zf, fma((double)jp, a.hb, a.b_lo), aw).d1;
            };
            if (!rtus_bracket_fix(j, a.m, d1_at, jl, jh)) continue;
            // Newton on dT / dbeta = 0 inside it; the inner alpha starts from the bracket's left end, then from the previous iterate
            double x, aw = alr[jl];
            const auto v = rtus_newton_min([&](double beta) {
                                               if constexpr (SKIP) {
                                                   const PipeTS r = pipe_T<POLY>(a, xa, za, xf, zf, beta, aw, L, vw);
                                                   vw = r.v;
                                                   return r;
                                               } else
                                                   return pipe_T<POLY>(a, xa, za, xf, zf, beta, aw);
                                           },
                                           fma((double)jl, a.hb, a.b_lo), fma((double)jh, a.hb, a.b_lo), 1e-12, x);
            // rule 1: the water segment L -> Q arrives from outside the circle; rule 2: the wall segment Q -> F keeps off the bore
            const double cx = v.qx - a.x_off, cz = v.qz;
            const bool outside = fma(v.qx - v.px, cx, (v.qz - v.pz) * cz) < 0.0;
            const double sx = xf - v.qx, sz = zf - v.qz, ss = fma(sx, sx, sz * sz);
            const double tc = fmin(fmax(-fma(cx, sx, cz * sz) / ss, 0.0), 1.0);
            const double nx = fma(tc, sx, cx), nz = fma(tc, sz, cz);
            const bool clear = SKIP || fma(nx, nx, nz * nz) >= rin2;      // (the skip leg's segments keep off the bore by construction)
            if (!(outside && clear && isfinite(v.t))) continue;
            if (isnan(best) || v.t < best) {
                best = v.t; bA = v.alpha; bB = x; tb = tk;
                if constexpr (SKIP) bG = v.gamma;
            }
        }
        a.tt[o] = best;
        if (a.alpha_out) a.alpha_out[o] = bA;
        if (a.beta_out) a.beta_out[o] = bB;
        if constexpr (SKIP) { if (k.gamma_out) k.gamma_out[o] = bG; }
    }
}

template <bool POLY>
__global__ void __launch_bounds__(RTUS_BLOCK) rtus_pipe_kernel(PipeArgs a)
{
    pipe_table<POLY, false>(a, PipeSkip{});
}

template <bool POLY>
__global__ void __launch_bounds__(RTUS_BLOCK) rtus_pipe_skip_kernel(PipeArgs a, PipeSkip k)
{
    pipe_table<POLY, true>(a, k);
}

// c_up > 0: the skip leg (P.c3 is c_down; gamma_out nullable); c_up == 0: the direct leg
static hipError_t launch_pipe(const rtus_lens& L, double a_lo, double a_hi, const rtus_pipe& P, double c_up, double b_lo, double b_hi,
                              int n_scan, const double* xe, const double* ze, int n_e, const double* xf, const double* zf, int n_f,
                              double* tt, double* alpha_out, double* beta_out, double* gamma_out, void* ws, hipStream_t s)
{
    PipeArgs a;
    a.k = make_lens_const<double>(L, a_lo, a_hi);
    a.a_lo = a_lo; a.a_hi = a_hi;
    a.gp_min = lens_gp_min(L);
    a.r_out = P.r_outer; a.r_in = P.r_inner; a.x_off = P.x_off; a.ic3 = 1.0 / P.c3;
    a.b_lo = b_lo; a.hb = (b_hi - b_lo) / (double)(n_scan - 1);
    a.k32f = (float)(P.c3 / L.c2); a.ic3f = (float)(1.0 / P.c3);
    a.m = n_scan; a.n_e = n_e; a.n_f = n_f;
    a.xe = xe; a.ze = ze; a.xf = xf; a.zf = zf; a.tt = tt; a.alpha_out = alpha_out; a.beta_out = beta_out;
    pipe_ws(ws, n_e, n_scan, &a);
    const long long gs = ((long long)n_e * n_scan + RTUS_BLOCK - 1) / RTUS_BLOCK;
    const long long gy = ((long long)n_e + PIPE_EB - 1) / PIPE_EB, gx = ((long long)n_f + RTUS_BLOCK - 1) / RTUS_BLOCK;
    if (gy > 65535 || gx > 0x7fffffffLL || gs > 0x7fffffffLL) return hipErrorInvalidValue;
    if (c_up > 0.0) {
        PipeSkip k;
        k.icu = 1.0 / c_up; k.aQ = acos(P.r_inner / P.r_outer); k.dQ = P.r_outer - P.r_inner;
        k.icuf = (float)k.icu; k.aQf = (float)k.aQ; k.dQf = (float)k.dQ;
        k.gamma_out = gamma_out;
        if (a.k.poly_trig) {
            hipLaunchKernelGGL(rtus_pipe_setup_kernel<true>, dim3((unsigned)gs), dim3(RTUS_BLOCK), 0, s, a);
            hipLaunchKernelGGL(rtus_pipe_skip_kernel<true>, dim3((unsigned)gx, (unsigned)gy), dim3(RTUS_BLOCK), 0, s, a, k);
        } else {
            hipLaunchKernelGGL(rtus_pipe_setup_kernel<false>, dim3((unsigned)gs), dim3(RTUS_BLOCK), 0, s, a);
            hipLaunchKernelGGL(rtus_pipe_skip_kernel<false>, dim3((unsigned)gx, (unsigned)gy), dim3(RTUS_BLOCK), 0, s, a, k);
        }
        return hipGetLastError();
    }
    if (a.k.poly_trig) {
        hipLaunchKernelGGL(rtus_pipe_setup_kernel<true>, dim3((unsigned)gs), dim3(RTUS_BLOCK), 0, s, a);
        hipLaunchKernelGGL(rtus_pipe_kernel<true>, dim3((unsigned)gx, (unsigned)gy), dim3(RTUS_BLOCK), 0, s, a);
    } else {
        hipLaunchKernelGGL(rtus_pipe_setup_kernel<false>, dim3((unsigned)gs), dim3(RTUS_BLOCK), 0, s, a);
        hipLaunchKernelGGL(rtus_pipe_kernel<false>, dim3((unsigned)gx, (unsigned)gy), dim3(RTUS_BLOCK), 0, s, a);
    }
    return hipGetLastError();
}

hipError_t rtus_launch_tt_pipe(const rtus_lens& L, double a_lo, double a_hi, const rtus_pipe& P, double b_lo, double b_hi, int n_scan,
                               const double* xe, const double* ze, int n_e, const double* xf, const double* zf, int n_f, double* tt,
                               double* alpha_out, double* beta_out, void* ws, hipStream_t s)
{
    return launch_pipe(L, a_lo, a_hi, P, 0.0, b_lo, b_hi, n_scan, xe, ze, n_e, xf, zf, n_f, tt, alpha_out, beta_out, nullptr, ws, s);
}

hipError_t rtus_launch_tt_pipe_skip(const rtus_lens& L, double a_lo, double a_hi, const rtus_pipe& P, double c_up, double b_lo, double b_hi,
                                    int n_scan, const double* xe, const double* ze, int n_e, const double* xf, const double* zf, int n_f,
                                    double* tt, double* alpha_out, double* beta_out, double* gamma_out, void* ws, hipStream_t s)
{
    return launch_pipe(L, a_lo, a_hi, P, c_up, b_lo, b_hi, n_scan, xe, ze, n_e, xf, zf, n_f, tt, alpha_out, beta_out, gamma_out, ws, s);
}
