// rtus_aniso.hip — travel times into a homogeneous ANISOTROPIC part (austenitic weld metal, cladding, CFRP): through one measured
// surface (rtus_tt_aniso_surface) and in contact (rtus_tt_aniso_direct).  NOT IN THE REFERENCE (parity unpinned): checked against
// tests/aniso_numpy.py, on an isotropic series against rtus_tt_surface and on an elliptical one against rtus_tt_layers.
//
// The medium is its GROUP SLOWNESS over the ray's direction, a Fourier series of period pi in the ray's angle psi from +z (down),
// positive towards +x:   S(psi) = a[0] + sum_{k=1..K} (a[k] cos 2k psi + b[k] sin 2k psi),  K <= 16.
// A leg from S(x) = (x, s(x)) to F has v = F - S(x), L = |v|, (sin psi, cos psi) = v / L — no angle is formed: cos 2 psi and
// sin 2 psi come from the unit vector, the harmonics from the rotation recurrence, every multiply-add written fma().
//
//   T(x)  = |E - S(x)| / c1 + L S(psi)
//   T2'   = -A S + S_psi Bq,                         A = sin psi + s' cos psi (= -L'),  Bq = s' sin psi - cos psi (= L psi')
//   T2''  = (S + S_psipsi) Bq^2 / L + s'' (S_psi sin psi - S cos psi)
//
// (T2: the second leg.  A' = -Bq^2 / L + s'' cos psi, Bq' = A Bq / L + s'' sin psi: the S_psi A Bq / L terms cancel.)  With S
// constant these are rtus_surface.hip's; everything else IS rtus_surface.hip's: its set-up kernel and workspace (the spline, the
// scan points at dx / 4), lanes = focal points, 8 elements per workgroup, the element's term per scan point in LDS, the fp32 sign
// scan of T', the three best brackets by a lower bound of their minimum's time, the fp64 bracket and safeguarded Newton of
// rtus_bracket.h.  The lane's term per scan point costs one series evaluation (8 fp32 operations per harmonic) where the isotropic
// kernel has one multiply; it depends on (focal point, scan point) only and is shared by the workgroup's elements.
//
// The scan's figure for a bracket is T(P_j+1) - (dx / 4) T'(P_j+1) as there: a lower bound of the minimum's time wherever T' is
// monotone between the root and P_j+1, whatever T is made of.  Its fp32 error: the series' (a few ulp per harmonic, weighted by
// |a_k| / a_0) on top of the isotropic kernel's 4e-6, so the third bracket is skipped against 8e-6.
//
// Guarantee and determinism: rtus_surface.hip's, word for word (an entry's bits depend on its element, focal point, the profile
// and the coefficients only).
#include "rtus_device.h"
#include "rtus_bracket.h"
#include "rtus_spline.h"

// no implicit contraction: the fma()s are written out, so every element slot's inlined copy of the arithmetic rounds alike
#pragma clang fp contract(off)

#define ANISO_EB 8          // elements per workgroup
#define ANISO_TILE 64       // scan points per LDS tile
#define ANISO_K 3           // brackets kept per (element, focal point)
#define ANISO_KMAX 16       // harmonics

// the series as the kernels get it: by value, read as scalars
struct AnisoSeries {
    double a[ANISO_KMAX + 1], b[ANISO_KMAX + 1];
    float4 f[ANISO_KMAX + 1];          // the fp32 scan's: (a_k, b_k, 2k b_k, -2k a_k), S = sum x c_k + y s_k, S_psi = sum z c_k + w s_k
    int K;
};

struct AnisoArgs {
    double x0, dx, hq, inv_dx, xend, c1, xo, zo;
    float ic1f, hqf;                   // 1 / c1, dx / 4
    int n_s, m, n_e, n_f;
    const double* __restrict__ xe;
    const double* __restrict__ ze;
    const double* __restrict__ xf;
    const double* __restrict__ zf;
    double* __restrict__ tt;
    double* __restrict__ xent;         // nullable
    const double* __restrict__ coef;
    const float4* __restrict__ pts;
    const double* __restrict__ smin;
};

// S, S_psi, S_psipsi at the direction (sn, cs) = (sin psi, cos psi)
struct AnisoS { double s, s1, s2; };
__device__ __forceinline__ AnisoS aniso_series(const AnisoSeries& ser, double sn, double cs)
{
    const double c2 = fma(cs, cs, -(sn * sn)), s2 = 2.0 * sn * cs;
    double ck = 1.0, sk = 0.0;                                          // cos 2k psi, sin 2k psi
    AnisoS o = {ser.a[0], 0.0, 0.0};
    for (int k = 1; k <= ser.K; ++k) {
        const double cn = fma(ck, c2, -(sk * s2)), sn1 = fma(sk, c2, ck * s2);
        ck = cn;
        sk = sn1;
        const double ak = ser.a[k], bk = ser.b[k], k2 = 2.0 * (double)k;
        const double p = fma(ak, ck, bk * sk), q = fma(bk, ck, -(ak * sk));
        o.s = o.s + p;
        o.s1 = fma(k2, q, o.s1);
        o.s2 = fma(-(k2 * k2), p, o.s2);
    }
    return o;
}

struct Tder { double t, d1, d2; };
__device__ __forceinline__ Tder aniso_T(const double* __restrict__ coef, int n_s, double x0, double dx, double inv_dx, double inv_c1,
                                        const AnisoSeries& ser, double xe, double ze, double xf, double zf, double x)
{
    double s, s1, s2;
    spline_eval(coef, n_s, x0, dx, inv_dx, x, s, s1, s2);
    const double ux = x - xe, uz = s - ze, vx = xf - x, vz = zf - s;
    const double q1 = fma(ux, ux, uz * uz), q2 = fma(vx, vx, vz * vz);
    const double r1 = 1.0 / sqrt(q1), r2 = 1.0 / sqrt(q2);
    const double l1 = q1 * r1, l2 = q2 * r2;
    const double A1 = fma(uz, s1, ux);                           // (S - E) . S'
    const double B = fma(s1, s1, 1.0);
    const double sn = vx * r2, cs = vz * r2;
    const AnisoS V = aniso_series(ser, sn, cs);
    const double A = fma(cs, s1, sn), Bq = fma(sn, s1, -cs);
    Tder o;
    o.t = fma(l1, inv_c1, l2 * V.s);
    o.d1 = fma(A1 * r1, inv_c1, fma(V.s1, Bq, -(A * V.s)));
    o.d2 = fma((fma(uz, s2, B) - A1 * A1 * r1 * r1) * r1, inv_c1, fma((V.s + V.s2) * Bq * Bq, r2, s2 * fma(V.s1, sn, -(V.s * cs))));
    return o;
}

__global__ void __launch_bounds__(RTUS_BLOCK) rtus_aniso_surface_kernel(AnisoArgs a, AnisoSeries ser)
{
    __shared__ float4 sp[ANISO_TILE];                                   // the tile's scan points
    __shared__ float4 sng[ANISO_TILE][ANISO_EB / 4];                    // -g1 / c1 per (point, element)
    __shared__ float4 st1[ANISO_TILE][ANISO_EB / 4];                    // |P - E| / c1 per (point, element)
    __shared__ float sxe[ANISO_EB], sze[ANISO_EB];
    const int tid = threadIdx.x;
    const int f = blockIdx.x * RTUS_BLOCK + tid;
    const int e0 = blockIdx.y * ANISO_EB;
    if (tid < ANISO_EB) {
        const int e = e0 + tid < a.n_e ? e0 + tid : a.n_e - 1;
        sxe[tid] = (float)(a.xe[e] - a.xo);
        sze[tid] = (float)(a.ze[e] - a.zo);
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
        }
    }
    const float xfr = fok ? (float)(xf - a.xo) : NAN, zfr = fok ? (float)(zf - a.zo) : NAN;

    float bt[ANISO_EB][ANISO_K];
    int bj[ANISO_EB][ANISO_K];
    bool neg[ANISO_EB];
#pragma unroll
    for (int e = 0; e < ANISO_EB; ++e) {
        neg[e] = false;
#pragma unroll
        for (int k = 0; k < ANISO_K; ++k) { bt[e][k] = INFINITY; bj[e][k] = -1; }
    }
    for (int base = 0; base < a.m; base += ANISO_TILE) {
        const int n = a.m - base < ANISO_TILE ? a.m - base : ANISO_TILE;
        __syncthreads();
        for (int i = tid; i < ANISO_TILE * ANISO_EB; i += RTUS_BLOCK) {
            const int j = i / ANISO_EB, e = i % ANISO_EB;
            const float4 P = j < n ? a.pts[base + j] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float ux = P.x - sxe[e], uz = P.y - sze[e];
            const float q = fmaf(uz, uz, ux * ux);
            const float r = __builtin_amdgcn_rsqf(q);
            ((float*)&sng[j][0])[e] = -(fmaf(uz, P.z, ux) * r) * a.ic1f;
            ((float*)&st1[j][0])[e] = q * r * a.ic1f;
            if (e == 0) sp[j] = P;
        }
        __syncthreads();
        for (int jj = 0; jj < n; ++jj) {
            const float4 P = sp[jj];
            // the lane's leg at P: T2' = -A S + S_psi Bq and its time L S, the series at the unit vector of F - P
            const float vx = xfr - P.x, vz = zfr - P.y;
            const float q = fmaf(vz, vz, vx * vx);
            const float r = __builtin_amdgcn_rsqf(q);
            const float sn = vx * r, cs = vz * r;
            const float c2 = fmaf(cs, cs, -(sn * sn)), s2 = 2.0f * sn * cs;
            float ck = 1.0f, sk = 0.0f, S = ser.f[0].x, S1 = 0.0f;
            for (int k = 1; k <= ser.K; ++k) {
                const float cn = fmaf(ck, c2, -(sk * s2)), sn1 = fmaf(sk, c2, ck * s2);
                ck = cn;
                sk = sn1;
                const float4 c = ser.f[k];
                S = fmaf(c.x, ck, fmaf(c.y, sk, S));
                S1 = fmaf(c.z, ck, fmaf(c.w, sk, S1));
            }
            const float g2 = fmaf(S1, fmaf(sn, P.z, -cs), -(fmaf(cs, P.z, sn) * S));     // T' = g2 - ng: T' > 0 <=> g2 > ng
            const float tin = q * r * S;
            const float4 ng0 = sng[jj][0], ng1 = sng[jj][1];
            const float ng[ANISO_EB] = {ng0.x, ng0.y, ng0.z, ng0.w, ng1.x, ng1.y, ng1.z, ng1.w};
            const int j = base + jj;
#pragma unroll
            for (int e = 0; e < ANISO_EB; ++e) {
                const bool pos = g2 > ng[e];
                if (pos && neg[e]) {                                    // - -> + between P_j-1 and P_j: a minimum
                    // T(P_j) - hq T'(P_j): a lower bound of the minimum's time
                    const float t = fmaf(ng[e] - g2, a.hqf, tin + ((const float*)&st1[jj][0])[e]);
                    RTUS_KEEP3(t, j - 1, bt[e], bj[e]);
                }
                neg[e] = !pos;                                          // (T' = 0 counts as -; NaN: never +)
            }
        }
    }
    if (f >= a.n_f) return;
    const double smin = a.smin[0];
    const double inv_c1 = 1.0 / a.c1;
#pragma unroll
    for (int e = 0; e < ANISO_EB; ++e) {
        const int row = e0 + e;
        if (row < a.n_e) {
            const size_t o = (size_t)row * a.n_f + f;
            const double xe = a.xe[row], ze = a.ze[row];
            auto T_at = [&](double x) { return aniso_T(a.coef, a.n_s, a.x0, a.dx, a.inv_dx, inv_c1, ser, xe, ze, xf, zf, x); };
            const bool ok = fok && ze < smin;
            // the least refined time over the kept brackets; the third: not when the lower bound of its minimum's time (less the
            // bound's fp32 error) is after the best refined time
            double best = NAN, bx = NAN;
            for (int k = 0; k < ANISO_K; ++k) {
                const int j = k == 0 ? bj[e][0] : (k == 1 ? bj[e][1] : bj[e][2]);
                if (!ok || j < 0 || (k >= 2 && (double)bt[e][2] > fma(8e-6, best, best))) continue;      // (best NaN: refined)
                int jl, jh;
                if (!rtus_bracket_fix(j, a.m, [&](int jp) { return T_at(fma((double)jp, a.hq, a.x0)).d1; }, jl, jh)) continue;
                double x;
                const Tder v = rtus_newton_min(T_at, fma((double)jl, a.hq, a.x0), fma((double)jh, a.hq, a.x0), 1e-10 * a.hq, x);
                if (isnan(best) || v.t < best) { best = v.t; bx = x; }
            }
            a.tt[o] = best;
            if (a.xent) a.xent[o] = bx;
        }
    }
}

// contact: the probe on the part, a straight ray, T = |F - E| S(psi)
__global__ void __launch_bounds__(RTUS_BLOCK) rtus_aniso_direct_kernel(const double* __restrict__ xe, const double* __restrict__ ze,
                                                                         const double* __restrict__ xf, const double* __restrict__ zf,
                                                                         int n_f, double* __restrict__ tt, AnisoSeries ser)
{
    const int f = blockIdx.x * RTUS_BLOCK + threadIdx.x;
    if (f >= n_f) return;
    const int e = blockIdx.y;
    const double ex = xe[e], ez = ze[e], fx = xf[f], fz = zf[f];
    const double vx = fx - ex, vz = fz - ez;
    const double q = fma(vx, vx, vz * vz);
    double t = NAN;
    if (isfinite(ex) && isfinite(ez) && isfinite(fx) && isfinite(fz)) {
        t = 0.0;
        if (q > 0.0) {
            const double r = 1.0 / sqrt(q);
            t = q * r * aniso_series(ser, vx * r, vz * r).s;
        }
    }
    tt[(size_t)e * n_f + f] = t;
}

// the series a call passes to its kernel
static AnisoSeries aniso_make(const double* a, const double* b, int K)
{
    AnisoSeries s = {};
    s.K = K;
    for (int k = 0; k <= K; ++k) {
        s.a[k] = a[k];
        s.b[k] = k ? b[k] : 0.0;
        s.f[k] = make_float4((float)s.a[k], (float)s.b[k], (float)(2.0 * k * s.b[k]), (float)(-2.0 * k * s.a[k]));
    }
    return s;
}

// what the entry points refuse: K outside 0 .. 16, a non-finite coefficient, a series that is not positive at one of 4096 uniform
// angles of its period
bool rtus_aniso_series_ok(const double* a, const double* b, int K)
{
    if (!a || !b || K < 0 || K > ANISO_KMAX) return false;
    for (int k = 0; k <= K; ++k)
        if (!isfinite(a[k]) || (k && !isfinite(b[k]))) return false;
    const int n = 4096;
    for (int i = 0; i < n; ++i) {
        const double psi = 3.14159265358979323846 * (double)i / (double)n;
        double s = a[0];
        for (int k = 1; k <= K; ++k) s += a[k] * cos(2.0 * k * psi) + b[k] * sin(2.0 * k * psi);
        if (!(s > 0.0) || !isfinite(s)) return false;
    }
    return true;
}

// the surface's set-up kernel, then the table kernel
hipError_t rtus_launch_tt_aniso_surface(double x0, double dx, const double* zs, int n_s, double c1, const double* a, const double* b, int K,
                                        const double* xe, const double* ze, int n_e, const double* xf, const double* zf, int n_f,
                                        double* tt, double* xent, void* ws, hipStream_t s)
{
    const long long gy = ((long long)n_e + ANISO_EB - 1) / ANISO_EB, gx = ((long long)n_f + RTUS_BLOCK - 1) / RTUS_BLOCK;
    if (gy > 65535 || gx > 0x7fffffffLL) return hipErrorInvalidValue;
    RtusSurfaceScan sc;
    const hipError_t err = rtus_launch_surface_setup_scan(zs, n_s, x0, dx, ws, &sc, s);
    if (err != hipSuccess) return err;
    AnisoArgs A = {};
    A.x0 = x0; A.dx = dx; A.hq = dx / 4.0; A.inv_dx = 1.0 / dx; A.xend = fma((double)(n_s - 1), dx, x0);
    A.c1 = c1; A.xo = sc.xo; A.zo = sc.zo;
    A.ic1f = (float)(1.0 / c1); A.hqf = (float)A.hq;
    A.n_s = n_s; A.m = sc.m; A.n_e = n_e; A.n_f = n_f;
    A.xe = xe; A.ze = ze; A.xf = xf; A.zf = zf; A.tt = tt; A.xent = xent;
    A.coef = sc.coef; A.pts = sc.pts; A.smin = sc.smin;
    hipLaunchKernelGGL(rtus_aniso_surface_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(RTUS_BLOCK), 0, s, A, aniso_make(a, b, K));
    return hipGetLastError();
}

hipError_t rtus_launch_tt_aniso_direct(const double* a, const double* b, int K, const double* xe, const double* ze, int n_e,
                                       const double* xf, const double* zf, int n_f, double* tt, hipStream_t s)
{
    const long long gx = ((long long)n_f + RTUS_BLOCK - 1) / RTUS_BLOCK;
    if (n_e > 65535 || gx > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rtus_aniso_direct_kernel, dim3((unsigned)gx, (unsigned)n_e), dim3(RTUS_BLOCK), 0, s, xe, ze, xf, zf, n_f, tt,
                       aniso_make(a, b, K));
    return hipGetLastError();
}
