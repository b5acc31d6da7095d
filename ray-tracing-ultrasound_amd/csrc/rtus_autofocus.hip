// rtus_autofocus.hip — measuring the surface profile from the FMC data that is later imaged ("adaptive TFM"): an analytic
// (complex) FMC by an FIR Hilbert transform, and an envelope image of the couplant above the part, reduced to the depth of the
// surface echo in every column.  NOT IN THE REFERENCE: checked against tests/autofocus_numpy.py.  Definitions in include/rtus.h
// (rtus_fmc_analytic, rtus_surface_find, rtus_echo_pick).
//
//   * rtus_analytic_kernel: one workgroup = RTUS_ANA_TILE samples of one A-scan plus the filter's halo in LDS; streams the FMC
//     (4 B in, 8 B out per sample) -> HBM roofline, a small share of the chain.  rtus_analytic_i16_kernel: the same on int16
//     samples (2 B in), also writing the Hilbert planes alone, pair-packed, for rtus_tfm_envelope_frames_hmc_i16.
//   * rtus_surface_find_kernel: the delay-and-sum core of rtus_das.h on complex samples, with straight-ray delays formed in the
//     kernel instead of read from a table: 16 B of L2 traffic per (pair, pixel).  The roof is the L2 gather rate, as for rtus_tfm
//     (DESIGN §4).
//   * rtus_echo_pick_kernel: one wave = one A-scan, lanes over the samples of its gate, 16-byte loads, a cross-lane arg-max that
//     keeps the first index; streams the gated part of the analytic FMC once -> HBM roofline.
#include "rtus_das.h"

// ---------------------------------------------------------------------------------------------- analytic FMC
// out[pair][n] = (x[n], sum_m h[m] x[n - m]).  h is odd-symmetric and zero at even m, so the sum is
// sum over odd m = 1..M of h[m] (x[n - m] - x[n + m]), in that order (fixed: the result does not depend on the launch).
#define RTUS_ANA_TILE 1024                                   // output samples per workgroup: 4 per lane
#define RTUS_ANA_MAX_HALF 127                                // M = (n_taps - 1) / 2, n_taps <= 255

struct AnaArgs {
    const float* __restrict__ x;                             // [n_pairs][n_t]
    float2* __restrict__ out;                                // [n_pairs][n_t]: (re, im)
    int n_t, n_tiles, M;
    float h[(RTUS_ANA_MAX_HALF + 1) / 2];                    // h[i] = tap 2 i + 1
};

__global__ __launch_bounds__(RTUS_BLOCK) void rtus_analytic_kernel(AnaArgs a)
{
    __shared__ float xs[RTUS_ANA_TILE + 2 * RTUS_ANA_MAX_HALF];
    const size_t pair = blockIdx.x / (unsigned)a.n_tiles;
    const int n0 = (int)(blockIdx.x % (unsigned)a.n_tiles) * RTUS_ANA_TILE;
    const float* rec = a.x + pair * (size_t)a.n_t;
    const int M = a.M;
    for (int i = threadIdx.x; i < RTUS_ANA_TILE + 2 * M; i += RTUS_BLOCK) {   // samples outside the record are zero
        const int n = n0 - M + i;
        xs[i] = (n >= 0 && n < a.n_t) ? rec[n] : 0.0f;
    }
    __syncthreads();
    float2* o = a.out + pair * (size_t)a.n_t;
#pragma unroll
    for (int q = 0; q < RTUS_ANA_TILE / RTUS_BLOCK; ++q) {
        const int l = q * RTUS_BLOCK + threadIdx.x, n = n0 + l;
        if (n >= a.n_t) break;
        const float* c = xs + l + M;                         // c[0] = x[n]
        float y = 0.0f;
        for (int i = 0; 2 * i + 1 <= M; ++i) y = fmaf(a.h[i], c[-(2 * i + 1)] - c[2 * i + 1], y);
        o[n] = make_float2(c[0], y);
    }
}

// the taps of every launcher of the transformer, formed in ONE place (fp64, rounded to fp32): -> M; h[i] = tap 2 i + 1
static int ana_taps(int n_taps, float h[(RTUS_ANA_MAX_HALF + 1) / 2])
{
    const int M = (n_taps - 1) / 2;
    for (int i = 0; i < (RTUS_ANA_MAX_HALF + 1) / 2; ++i) {
        const int m = 2 * i + 1;                             // h[m] = 2 / (pi m) w[m], w the Hamming window over -M..M
        h[i] = m <= M ? (float)(2.0 / (M_PI * m) * (0.54 + 0.46 * cos(M_PI * m / M))) : 0.0f;
    }
    return M;
}

hipError_t rtus_launch_fmc_analytic(const float* fmc, long long n_pairs, int n_t, int n_taps, float2* out, hipStream_t s)
{
    AnaArgs a;
    a.x = fmc; a.out = out; a.n_t = n_t;
    a.n_tiles = (n_t + RTUS_ANA_TILE - 1) / RTUS_ANA_TILE;
    a.M = ana_taps(n_taps, a.h);
    hipLaunchKernelGGL(rtus_analytic_kernel, dim3((unsigned)(n_pairs * a.n_tiles)), dim3(RTUS_BLOCK), 0, s, a);
    return hipGetLastError();
}

// The transformer on INT16 samples (include/rtus.h: rtus_fmc_analytic_i16, rtus_fmc_hilbert_pairs_i16_dev): rtus_analytic_kernel's
// tile, halo and sum on the samples converted to fp32 when the tile is filled — the conversion is exact and so is the difference
// of two converted values (|d| <= 65535 < 2^24), so y has the bits of rtus_analytic_kernel on the float32 copy.  One body, two
// output forms:
//   PAIRS = false: out [n_rows][n_t][2] = (x, Hx) of the n_rows A-scans of the stack, rtus_analytic_kernel's output;
//   PAIRS = true:  the Hilbert planes ALONE in the float32 pair-packed layout of rtus_tfm_frames_hmc_dev, out [n_fpairs][n_scans][n_t][2]:
//                  plane c of pair p is H of frame 2 p + c.  A workgroup takes the same tile of BOTH frames of a pair and stores
//                  float2 (8-byte stores, contiguous per wave); the absent frame of an odd stack fills its tile with zeros, whose
//                  sum is fmaf(h, +0 - +0, +0) = +0.0 for either sign of h: the plane pack_frames writes.
struct AnaI16Args {
    const short* __restrict__ x;                             // [n_frames][n_scans][n_t]
    float2* __restrict__ out;
    int n_t, n_tiles, M;
    int n_frames, n_scans;                                   // (PAIRS only)
    float h[(RTUS_ANA_MAX_HALF + 1) / 2];                    // h[i] = tap 2 i + 1
};

template <bool PAIRS>
__global__ __launch_bounds__(RTUS_BLOCK) void rtus_analytic_i16_kernel(AnaI16Args a)
{
    constexpr int P = PAIRS ? 2 : 1;
    __shared__ float xs[P][RTUS_ANA_TILE + 2 * RTUS_ANA_MAX_HALF];
    const size_t row = blockIdx.x / (unsigned)a.n_tiles;     // PAIRS: pair * n_scans + scan; else the A-scan
    const int n0 = (int)(blockIdx.x % (unsigned)a.n_tiles) * RTUS_ANA_TILE;
    const int M = a.M;
#pragma unroll
    for (int c = 0; c < P; ++c) {
        size_t scan = row;
        bool have = true;
        if constexpr (PAIRS) {
            const size_t frame = 2 * (row / (unsigned)a.n_scans) + c;
            have = frame < (size_t)a.n_frames;               // (an absent frame's record does not exist and is not read)
            scan = frame * (unsigned)a.n_scans + row % (unsigned)a.n_scans;
        }
        const short* rec = a.x + scan * (size_t)a.n_t;
        for (int i = threadIdx.x; i < RTUS_ANA_TILE + 2 * M; i += RTUS_BLOCK) {   // samples outside the record are zero
            const int n = n0 - M + i;
            xs[c][i] = (have && n >= 0 && n < a.n_t) ? (float)rec[n] : 0.0f;
        }
    }
    __syncthreads();
    float2* o = a.out + row * (size_t)a.n_t;
#pragma unroll
    for (int q = 0; q < RTUS_ANA_TILE / RTUS_BLOCK; ++q) {
        const int l = q * RTUS_BLOCK + threadIdx.x, n = n0 + l;
        if (n >= a.n_t) break;
        float y[P];
#pragma unroll
        for (int c = 0; c < P; ++c) {
            const float* t = xs[c] + l + M;                  // t[0] = x[n]
            y[c] = 0.0f;
            for (int i = 0; 2 * i + 1 <= M; ++i) y[c] = fmaf(a.h[i], t[-(2 * i + 1)] - t[2 * i + 1], y[c]);
        }
        if constexpr (PAIRS) o[n] = make_float2(y[0], y[1]);
        else o[n] = make_float2(xs[0][l + M], y[0]);
    }
}

// n_frames stacks of n_scans A-scans; pairs: the pair-packed Hilbert planes, else (x, Hx) of every A-scan.  The C entries have
// checked that the grid fits.
hipError_t rtus_launch_fmc_analytic_i16(const short* stack, int n_frames, long long n_scans, int n_t, int n_taps, bool pairs, float* out,
                                        hipStream_t s)
{
    AnaI16Args a;
    a.x = stack; a.out = (float2*)out; a.n_t = n_t;
    a.n_tiles = (n_t + RTUS_ANA_TILE - 1) / RTUS_ANA_TILE;
    a.M = ana_taps(n_taps, a.h);
    a.n_frames = n_frames; a.n_scans = (int)n_scans;
    const long long rows = pairs ? (n_frames + 1LL) / 2 * n_scans : n_frames * n_scans;
    const dim3 grid((unsigned)(rows * a.n_tiles)), block(RTUS_BLOCK);
    if (pairs) hipLaunchKernelGGL(rtus_analytic_i16_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(rtus_analytic_i16_kernel<false>, grid, block, 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- couplant envelope + peak
// A[k][j] = | sum_tx sum_rx a[tx][rx](s) |, s = (|E_tx - P| + |E_rx - P|) / c1 fs - t0 fs, P = (x0 + k dx, z_lo + j dz); real
// and imaginary parts interpolated linearly and separately, rtus_tfm's edge rules.  Then the first index of the column's
// maximum and a parabolic step.
//
// One workgroup = one column, lanes over depths (n_z > 256: the workgroup walks the column in chunks of 256).  Each element's
// half of the sample position (fp64, rounded once to fp32, as rtus_tfm's tfm_tau) sits in LDS for a tile of RTUS_SF_TILE
// elements; the workgroup order (here: of the columns), the 16-byte loads and the gather loop are rtus_das.h's.
#define RTUS_SF_TILE 64
#define RTUS_SF_MAX_Z 1024

struct SfArgs {
    const float* __restrict__ a;         // [n_e][n_e][n_t][2]
    const double* __restrict__ xe;
    const double* __restrict__ ze;
    double* __restrict__ z_peak;         // [n_s]
    float* __restrict__ amp;             // [n_s]
    float* __restrict__ image;           // [n_s][n_z] or null
    int n_e, n_t, n_s, n_z;
    double c1, fs, half_t0s, x0, dx, z_lo, dz;
};

__device__ __forceinline__ float sf_tau(double xe, double ze, double px, double pz, double c1, double fs, double half_t0s)
{
    const double ux = xe - px, uz = ze - pz;
    return das_clamp((float)(sqrt(ux * ux + uz * uz) / c1 * fs - half_t0s));   // (positions are finite; absurd ones read nothing)
}

__global__ __launch_bounds__(RTUS_BLOCK) void rtus_surface_find_kernel(SfArgs a)
{
    __shared__ float tau[RTUS_SF_TILE][RTUS_BLOCK];          // 64 KB
    __shared__ float col[RTUS_SF_MAX_Z];                     // the column's amplitudes, for the parabolic step
    __shared__ float red_v[RTUS_BLOCK];
    __shared__ int red_i[RTUS_BLOCK];
    const int k = das_workgroup();                           // neighbouring columns read the same sample windows
    const int t = threadIdx.x;
    const double px = a.x0 + k * a.dx;
    const size_t pair_len = (size_t)a.n_t * 2;               // floats per analytic A-scan
    const bool tx_in_tile = a.n_e <= RTUS_SF_TILE;
    float best = -1.0f;                                      // this lane's maximum (first index), and whether it saw a NaN / inf
    int best_j = a.n_z;
    bool bad = false;
    for (int j0 = 0; j0 < a.n_z; j0 += RTUS_BLOCK) {
        const int j_raw = j0 + t;
        const bool live = j_raw < a.n_z;
        const int j = live ? j_raw : a.n_z - 1;
        const double pz = a.z_lo + j * a.dz;
        float re = 0.0f, im = 0.0f;
        for (int r0 = 0; r0 < a.n_e; r0 += RTUS_SF_TILE) {
            const int nr = min(RTUS_SF_TILE, a.n_e - r0);
            __syncthreads();                                 // the previous tile is no longer read
            for (int r = 0; r < nr; ++r) tau[r][t] = sf_tau(a.xe[r0 + r], a.ze[r0 + r], px, pz, a.c1, a.fs, a.half_t0s);
            __syncthreads();
            for (int tx = 0; tx < a.n_e; ++tx) {
                const float tt = tx_in_tile ? tau[tx][t] : sf_tau(a.xe[tx], a.ze[tx], px, pz, a.c1, a.fs, a.half_t0s);
                das_gather<2>(a.a + ((size_t)tx * a.n_e + r0) * pair_len, pair_len, a.n_t, tt, tau, t, nr,
                              [&](int, das_u32x4 v, float w) {
                                  const float2 p = das_lerp(v, w);
                                  re += p.x;
                                  im += p.y;
                              });
            }
        }
        const float A = sqrtf(re * re + im * im);
        if (live) {
            col[j] = A;
            if (a.image) a.image[(size_t)k * a.n_z + j] = A;
            bad |= !(A <= 3.402823466e38f);                  // NaN or inf
            if (A > best) { best = A; best_j = j; }          // ascending j: strict > keeps the first index
        }
    }
    red_v[t] = best;
    red_i[t] = bad ? -1 : best_j;                            // -1: this lane saw a non-finite amplitude
    for (int h = RTUS_BLOCK / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (t < h) {
            const float v1 = red_v[t], v2 = red_v[t + h];
            const int i1 = red_i[t], i2 = red_i[t + h];
            if (i1 < 0 || i2 < 0) red_i[t] = -1;
            else if (v2 > v1 || (v2 == v1 && i2 < i1)) { red_v[t] = v2; red_i[t] = i2; }
        }
    }
    __syncthreads();
    if (t == 0) {
        const float m = red_v[0];
        const int js = red_i[0];
        double z = NAN;
        if (js > 0 && js < a.n_z - 1 && m > 0.0f) {         // inside the window, a finite, non-zero maximum
            const double am = col[js - 1], a0 = col[js], ap = col[js + 1];
            double d = (am - ap) / (2.0 * (am - 2.0 * a0 + ap)); // am < a0 (first index of the maximum), ap <= a0: denominator < 0
            d = fmin(fmax(d, -0.5), 0.5);
            z = a.z_lo + (js + d) * a.dz;
        }
        a.z_peak[k] = z;
        a.amp[k] = js < 0 ? NAN : m;
    }
}

hipError_t rtus_launch_surface_find(const float* an, int n_e, int n_t, double fs, double t0, const double* xe, const double* ze,
                                    double c1, double x0, double dx, int n_s, double z_lo, double dz, int n_z, double* z_peak,
                                    float* amp, float* image, hipStream_t s)
{
    SfArgs a;
    a.a = an; a.xe = xe; a.ze = ze; a.z_peak = z_peak; a.amp = amp; a.image = image;
    a.n_e = n_e; a.n_t = n_t; a.n_s = n_s; a.n_z = n_z;
    a.c1 = c1; a.fs = fs; a.half_t0s = 0.5 * t0 * fs; a.x0 = x0; a.dx = dx; a.z_lo = z_lo; a.dz = dz;
    hipLaunchKernelGGL(rtus_surface_find_kernel, dim3(n_s), dim3(RTUS_BLOCK), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- echo time of every pair
// t_pick[pair] = t0 + (j* + d) / fs, j* the first index of the maximum of |a[pair][.]| over the samples of the pair's gate and d
// rtus_surface_find's parabolic step.  The magnitude is fp32, every operation rounded on its own (no fused multiply-add), so that
// it can be restated bit for bit: sqrt(re * re + im * im), the root correctly rounded.
//
// One wave = one A-scan (RTUS_BLOCK / RTUS_WAVE per workgroup, no barrier).  Lane l takes the sample pairs (2 l, 2 l + 1) of a
// trip of 128 samples, counted from the 16-byte boundary at or below the gate's first sample; four trips' loads are issued before
// the first is used.  A 16-byte load is issued only where both of its samples are inside the gate (so nothing outside the caller's
// block is read); the one or two half-filled loads at the gate's ends are 8-byte loads.
#define RTUS_PICK_UNROLL 4

struct PickArgs {
    const float2* __restrict__ a;        // [n_pairs][n_t]
    const double* __restrict__ g_lo;     // [n_pairs] or null
    const double* __restrict__ g_hi;     // [n_pairs] or null
    double* __restrict__ t_pick;         // [n_pairs]
    float* __restrict__ amp;             // [n_pairs]
    long long n_pairs;
    int n_t;
    double fs, t0, t_lo, t_hi;
};

__device__ __forceinline__ float pick_mag(float re, float im)
{
#pragma clang fp contract(off)                               // re * re + im * im must not become a fused multiply-add
    const float p = re * re, q = im * im;
    // v_sqrt_f32 is good to 1 ulp only.  The fp64 root is correctly rounded (rtus_trig.h), and rounding it once more to fp32 is
    // innocuous for a square root: 53 >= 2 * 24 + 2 bits.
    return (float)rtus_sqrt((double)(p + q));
}

// one sample into a lane's running maximum: ascending index within a lane, strict > keeps the first
__device__ __forceinline__ void pick_take(float m, int i, float& best, int& best_i, bool& bad)
{
    bad |= !(m <= 3.402823466e38f);                          // NaN or inf
    if (m > best) { best = m; best_i = i; }
}

// the samples i, i + 1 (rec + i 16-byte aligned), each only where it lies inside [i_lo, i_hi]
__device__ __forceinline__ void pick_guarded(const float2* rec, int i, int i_lo, int i_hi, float& best, int& best_i, bool& bad)
{
    const bool in0 = i >= i_lo && i <= i_hi, in1 = i + 1 >= i_lo && i + 1 <= i_hi;
    if (in0 && in1) {
        const float4 v = *(const float4*)(rec + i);
        pick_take(pick_mag(v.x, v.y), i, best, best_i, bad);
        pick_take(pick_mag(v.z, v.w), i + 1, best, best_i, bad);
    } else if (in0) {
        const float2 v = rec[i];
        pick_take(pick_mag(v.x, v.y), i, best, best_i, bad);
    } else if (in1) {
        const float2 v = rec[i + 1];
        pick_take(pick_mag(v.x, v.y), i + 1, best, best_i, bad);
    }
}

__global__ __launch_bounds__(RTUS_BLOCK) void rtus_echo_pick_kernel(PickArgs a)
{
    const long long pair = (long long)blockIdx.x * (RTUS_BLOCK / RTUS_WAVE) + (threadIdx.x / RTUS_WAVE);
    if (pair >= a.n_pairs) return;                           // (whole waves: no barrier below)
    const int lane = threadIdx.x % RTUS_WAVE;
    // the gate in samples: t_lo <= t0 + i / fs <= t_hi, inside the record
    double lo = ceil(((a.g_lo ? a.g_lo[pair] : a.t_lo) - a.t0) * a.fs);
    double hi = floor(((a.g_hi ? a.g_hi[pair] : a.t_hi) - a.t0) * a.fs);
    const bool ordered = lo <= hi;                           // (false for a NaN bound: fmax / fmin below would drop it)
    lo = fmax(lo, 0.0);
    hi = fmin(hi, (double)(a.n_t - 1));
    const bool open = ordered && lo <= hi;                   // (false for an empty gate and for a gate outside the record)
    const int i_lo = open ? (int)lo : 0, i_hi = open ? (int)hi : -1;
    const float2* rec = a.a + pair * (long long)a.n_t;
    float best = -1.0f;
    int best_i = a.n_t;
    bool bad = false;
    const int s0 = i_lo - (int)(((uintptr_t)(rec + i_lo) >> 3) & 1);      // rec + s0 is 16-byte aligned; s0 >= i_lo - 1
    const int step = 2 * RTUS_WAVE;
    int i = s0 + 2 * lane;
    if (s0 < i_lo) {                                         // the gate starts on an odd boundary: lane 0 holds the sample before it
        pick_guarded(rec, i, i_lo, i_hi, best, best_i, bad);
        i += step;
    }
    // full trips: every lane's two samples of all RTUS_PICK_UNROLL trips lie inside the gate (a wave-uniform test)
    for (; (long long)(i - 2 * lane) + RTUS_PICK_UNROLL * step - 1 <= i_hi; i += RTUS_PICK_UNROLL * step) {
        float4 v[RTUS_PICK_UNROLL];
#pragma unroll
        for (int q = 0; q < RTUS_PICK_UNROLL; ++q) v[q] = *(const float4*)(rec + i + q * step);
#pragma unroll
        for (int q = 0; q < RTUS_PICK_UNROLL; ++q) {
            pick_take(pick_mag(v[q].x, v[q].y), i + q * step, best, best_i, bad);
            pick_take(pick_mag(v[q].z, v[q].w), i + q * step + 1, best, best_i, bad);
        }
    }
    for (; i <= i_hi; i += step) pick_guarded(rec, i, i_lo, i_hi, best, best_i, bad);      // the tail
    // cross-lane arg-max, the first index among equal maxima; every lane ends with the wave's result
    int key = bad ? -1 : best_i;                             // -1: a non-finite magnitude inside the gate
#pragma unroll
    for (int h = RTUS_WAVE / 2; h > 0; h >>= 1) {
        const float v2 = __shfl_xor(best, h, RTUS_WAVE);
        const int k2 = __shfl_xor(key, h, RTUS_WAVE);
        if (key < 0 || k2 < 0) key = -1;
        else if (v2 > best || (v2 == best && k2 < key)) { best = v2; key = k2; }
    }
    if (lane == 0) {
        double t = NAN;
        if (key > i_lo && key < i_hi && best > 0.0f) {       // inside the gate, a finite, non-zero maximum
            const float2 vm = rec[key - 1], vp = rec[key + 1];
            const double am = pick_mag(vm.x, vm.y), a0 = best, ap = pick_mag(vp.x, vp.y);
            double d = (am - ap) / (2.0 * (am - 2.0 * a0 + ap));         // am < a0, ap <= a0: denominator < 0
            d = fmin(fmax(d, -0.5), 0.5);
            t = a.t0 + ((double)key + d) / a.fs;
        }
        a.t_pick[pair] = t;
        a.amp[pair] = (key < 0 || !open) ? NAN : best;
    }
}

hipError_t rtus_launch_echo_pick(const float* an, long long n_pairs, int n_t, double fs, double t0, double t_lo, double t_hi,
                                 const double* g_lo, const double* g_hi, double* t_pick, float* amp, hipStream_t s)
{
    PickArgs a;
    a.a = (const float2*)an; a.g_lo = g_lo; a.g_hi = g_hi; a.t_pick = t_pick; a.amp = amp;
    a.n_pairs = n_pairs; a.n_t = n_t; a.fs = fs; a.t0 = t0; a.t_lo = t_lo; a.t_hi = t_hi;
    const int per = RTUS_BLOCK / RTUS_WAVE;
    hipLaunchKernelGGL(rtus_echo_pick_kernel, dim3((unsigned)((n_pairs + per - 1) / per)), dim3(RTUS_BLOCK), 0, s, a);
    return hipGetLastError();
}
