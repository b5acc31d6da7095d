// rtus_tfm.hip — the consumers of a travel-time table: transmit focal laws and a total-focusing-
// method (TFM) delay-and-sum beamformer over full-matrix-capture (FMC) data.  NOT IN THE REFERENCE (it stops at the
// travel times, main_rt.py:497-504): checked against the NumPy restatement oracle/tfm_numpy.py on synthetic
// point-scatterer data.
//
// Unlike every other kernel of this library these two are bound by memory, not by VALU issue:
//   * the focal-law kernels stream the table: 8 B read and 8 B written per entry (apertures up to 512 elements: the
//     column lives in registers between the maximum and the subtraction; larger ones re-read it: 24 B) -> HBM roofline;
//   * rtus_tfm_kernel gathers two neighbouring fp32 samples per (tx, rx, focal point) from the A-scan of that pair:
//     8 B of L2 traffic per pair and focal point.  The FMC block (n_tx n_rx n_t 4 B: 34 MB at 64 x 64 x 2048) is read
//     from HBM about once per launch and then lives in L2 / Infinity Cache, so the bound is the L2 gather rate
//     (MI355X_MICROARCH.md "Indexed rows": 17-19 TB/s chip-wide for rows shared by every workgroup), not HBM.
#include "rtus_das.h"

// ---------------------------------------------------------------------------------------------- focal laws
// delays[e][f] = max_e' tt[e'][f] - tt[e][f]: what element e must wait so that all wavefronts reach f together.
// NaN (no ray path) is ignored by the maximum and stays NaN in the result; a column without any path is all NaN.
// One workgroup = 256 consecutive focal points x all elements, two passes over its strip (coalesced 2 KB rows).
__global__ __launch_bounds__(RTUS_BLOCK) void rtus_focal_delays_kernel(const double* tt, int n_e, int n_f,
                                                                        double* delays)   // may alias tt (in place)
{
    const int f = blockIdx.x * RTUS_BLOCK + threadIdx.x;
    if (f >= n_f) return;
    const size_t nf = (size_t)n_f;
    double m = -INFINITY;
    int e = 0;
    for (; e + 4 <= n_e; e += 4) {                         // four loads in flight per lane
        const double a = tt[(size_t)e * nf + f], b = tt[(size_t)(e + 1) * nf + f], c = tt[(size_t)(e + 2) * nf + f],
                     d = tt[(size_t)(e + 3) * nf + f];
        m = fmax(fmax(m, a), fmax(b, fmax(c, d)));         // fmax ignores NaN operands
    }
    for (; e < n_e; ++e) m = fmax(m, tt[(size_t)e * nf + f]);
    m = (m == -INFINITY) ? NAN : m;                        // no element reaches this focal point
    for (e = 0; e < n_e; ++e) {
        const size_t o = (size_t)e * nf + f;
        delays[o] = m - tt[o];                             // NaN - x and x - NaN stay NaN
    }
}

// The same for apertures of up to 8 x RTUS_FD_ROWS elements, reading the table ONCE: a workgroup = 32 focal points x 8 row
// groups; a thread keeps its <= RTUS_FD_ROWS entries of one column in registers, the eight partial maxima of a column meet
// in LDS, and the thread subtracts and writes from its registers (in place is safe: a thread only writes what it has
// read).  16 B of HBM traffic per entry instead of 24 (measured on the 537 MB configs[2] table: the strip a workgroup of
// the two-pass kernel comes back to has long left the caches).  Lanes 0-31 of a wave are 32 neighbouring columns of one
// row, lanes 32-63 the same columns 1/8 of the aperture further down: two 256-byte segments per load.
#define RTUS_FD_ROWS 64
template <int ROWS>
__global__ __launch_bounds__(RTUS_BLOCK) void rtus_focal_delays_once_kernel(const double* tt, int n_e, int n_f, double* delays)
{
    __shared__ double part[8][32];
    const int c = threadIdx.x & 31, g = threadIdx.x >> 5;             // column inside the tile, row group
    const int f_raw = blockIdx.x * 32 + c;
    const bool live = f_raw < n_f;
    const int f = live ? f_raw : n_f - 1;
    const int per = (n_e + 7) / 8;                                     // rows per group (<= ROWS)
    const int e0 = g * per;
    const size_t nf = (size_t)n_f;
    double v[ROWS];
    double m = -INFINITY;
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
        const int e = e0 + k;
        v[k] = (k < per && e < n_e) ? tt[(size_t)e * nf + f] : NAN;   // NaN: ignored by fmax, never stored
        m = fmax(m, v[k]);
    }
    part[g][c] = m;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) m = fmax(m, part[j][c]);
    m = (m == -INFINITY) ? NAN : m;                                    // no element reaches this focal point
    if (!live) return;
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
        const int e = e0 + k;
        if (k < per && e < n_e) delays[(size_t)e * nf + f] = m - v[k];
    }
}

hipError_t rtus_launch_focal_delays(const double* tt, int n_e, int n_f, double* delays, hipStream_t s)
{
    const int per = (n_e + 7) / 8;
    const dim3 grid1((n_f + 31) / 32), block(RTUS_BLOCK);
    if (per <= 8) hipLaunchKernelGGL(rtus_focal_delays_once_kernel<8>, grid1, block, 0, s, tt, n_e, n_f, delays);
    else if (per <= 16) hipLaunchKernelGGL(rtus_focal_delays_once_kernel<16>, grid1, block, 0, s, tt, n_e, n_f, delays);
    else if (per <= 32) hipLaunchKernelGGL(rtus_focal_delays_once_kernel<32>, grid1, block, 0, s, tt, n_e, n_f, delays);
    else if (per <= RTUS_FD_ROWS) hipLaunchKernelGGL(rtus_focal_delays_once_kernel<RTUS_FD_ROWS>, grid1, block, 0, s, tt, n_e, n_f, delays);
    else hipLaunchKernelGGL(rtus_focal_delays_kernel, dim3((n_f + RTUS_BLOCK - 1) / RTUS_BLOCK), block, 0, s, tt, n_e, n_f, delays);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- TFM delay-and-sum
// image[f] = sum over (tx, rx) of the A-scan fmc[tx][rx][.] linearly interpolated at the sample position
// (tt_tx[tx][f] + tt_rx[rx][f] - t0) fs.  Samples outside the record count as zero; pairs without a ray path (NaN
// travel time) contribute nothing.
//
// One workgroup = 256 focal points, a receive tile of RTUS_TFM_RX_TILE elements' delays in LDS, 8 bytes gathered per pair and
// focal point: the delay-and-sum core of rtus_das.h, where the workgroup order, the loads' edge rules and the gather loop are
// described.
#define RTUS_TFM_RX_TILE 64

struct TfmArgs {
    const float* __restrict__ fmc;       // [n_tx][n_rx][n_t]
    const double* __restrict__ tt_tx;    // [n_tx][n_f]
    const double* __restrict__ tt_rx;    // [n_rx][n_f]
    float* __restrict__ image;           // [n_f]
    int n_tx, n_rx, n_t, n_f;
    double fs;                           // samples per second
    double half_t0s;                     // t0 * fs / 2: each of the pair's two delays carries half of the time origin
};

// what TfmArgs, TfmaArgs and TfmwArgs have in common (the fields above but image), filled once
template <class Args>
static Args tfm_args(const float* fmc, int n_tx, int n_rx, int n_t, double fs, double t0, const double* tt_tx, const double* tt_rx, int n_f)
{
    Args a;
    a.fmc = fmc; a.tt_tx = tt_tx; a.tt_rx = tt_rx;
    a.n_tx = n_tx; a.n_rx = n_rx; a.n_t = n_t; a.n_f = n_f;
    a.fs = fs; a.half_t0s = 0.5 * t0 * fs;
    return a;
}

__global__ __launch_bounds__(RTUS_BLOCK) void rtus_tfm_kernel(TfmArgs a)
{
    __shared__ float tau_rx[RTUS_TFM_RX_TILE][RTUS_BLOCK];           // 64 KB: 2 workgroups per CU; a 64-element receive
                                                                      // aperture is ONE tile: the transmit delays are read once
    const int f_raw = das_workgroup() * RTUS_BLOCK + threadIdx.x;
    const bool live = f_raw < a.n_f;
    const int f = live ? f_raw : a.n_f - 1;
    const size_t nf = (size_t)a.n_f;
    float acc = 0.0f;
    for (int r0 = 0; r0 < a.n_rx; r0 += RTUS_TFM_RX_TILE) {
        const int nr = min(RTUS_TFM_RX_TILE, a.n_rx - r0);
        __syncthreads();                                              // the previous tile is no longer read
        for (int r = 0; r < nr; ++r) tau_rx[r][threadIdx.x] = tfm_tau(a.tt_rx[(size_t)(r0 + r) * nf + f], a.fs, a.half_t0s);
        __syncthreads();
        // one table for both legs and the whole receive aperture in this tile: the transmit delay IS a row of the tile
        const bool tx_in_tile = a.tt_tx == a.tt_rx && a.n_tx == a.n_rx && a.n_rx <= RTUS_TFM_RX_TILE;
        for (int tx = 0; tx < a.n_tx; ++tx) {
            const float tt = tx_in_tile ? tau_rx[tx][threadIdx.x] : tfm_tau(a.tt_tx[(size_t)tx * nf + f], a.fs, a.half_t0s);
            das_gather<1>(a.fmc + ((size_t)tx * a.n_rx + r0) * (size_t)a.n_t, (size_t)a.n_t, a.n_t, tt, tau_rx, threadIdx.x, nr,
                          [&](int, das_u32x2 v, float w) { acc += das_lerp(v, w); });
        }
    }
    if (live) a.image[f] = acc;
}

hipError_t rtus_launch_tfm(const float* fmc, int n_tx, int n_rx, int n_t, double fs, double t0, const double* tt_tx,
                           const double* tt_rx, int n_f, float* image, hipStream_t s)
{
    TfmArgs a = tfm_args<TfmArgs>(fmc, n_tx, n_rx, n_t, fs, t0, tt_tx, tt_rx, n_f);
    a.image = image;
    hipLaunchKernelGGL(rtus_tfm_kernel, dim3((n_f + RTUS_BLOCK - 1) / RTUS_BLOCK), dim3(RTUS_BLOCK), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- envelope TFM + coherence factor
// The same delay-and-sum over an analytic (complex) FMC: S[f] = sum over (tx, rx) of a[tx][rx] at rtus_tfm's sample position, real
// and imaginary parts interpolated separately with rtus_tfm's arithmetic, edge rules and order — so S.re is
// rtus_tfm on the real parts and S.im rtus_tfm on the imaginary parts, bit for bit.  With CF, also E[f] = sum over the pairs of
// |a(s)|^2 and N[f] = T[f] R[f], the legs with a path counted while the delays are formed (none of it in the gather loop but two
// FMAs); cf = |S|^2 / (N E) in fp64.  Definition: include/rtus.h (rtus_tfm_analytic).  16 B of L2 traffic per (pair, focal point).
struct TfmaArgs {
    const float* __restrict__ fmc;       // [n_tx][n_rx][n_t][2]
    const double* __restrict__ tt_tx;    // [n_tx][n_f]
    const double* __restrict__ tt_rx;    // [n_rx][n_f]
    float2* __restrict__ image;          // [n_f]
    float* __restrict__ cf;              // [n_f] (read by the CF instantiation only)
    int n_tx, n_rx, n_t, n_f;
    double fs, half_t0s;
};

// Lerp: the step from a loaded pair to the interpolated sample p (rtus_das.h): DasLerp, or DasIq for rtus_tfm_iq_kernel
// (the arguments by value: by reference rtus_tfm_analytic_kernel's register allocation moves, scripts/asm_body_digest.py)
template <bool CF, class Lerp>
__device__ __forceinline__ void tfma_body(TfmaArgs a, float (*tau_rx)[RTUS_BLOCK], Lerp lerp)
{
    const int f_raw = das_workgroup() * RTUS_BLOCK + threadIdx.x;
    const bool live = f_raw < a.n_f;
    const int f = live ? f_raw : a.n_f - 1;
    const size_t nf = (size_t)a.n_f;
    const size_t pair_len = (size_t)a.n_t * 2;                        // floats per analytic A-scan
    const bool tx_in_tile = a.tt_tx == a.tt_rx && a.n_tx == a.n_rx && a.n_rx <= RTUS_TFM_RX_TILE;
    float re = 0.0f, im = 0.0f, en = 0.0f;
    int n_tx_ok = 0, n_rx_ok = 0;                                     // T[f], R[f] (CF only)
    for (int r0 = 0; r0 < a.n_rx; r0 += RTUS_TFM_RX_TILE) {
        const int nr = min(RTUS_TFM_RX_TILE, a.n_rx - r0);
        __syncthreads();                                              // the previous tile is no longer read
        for (int r = 0; r < nr; ++r) {
            const float v = tfm_tau(a.tt_rx[(size_t)(r0 + r) * nf + f], a.fs, a.half_t0s);
            tau_rx[r][threadIdx.x] = v;
            if (CF) n_rx_ok += tfm_has_path(v);
        }
        __syncthreads();
        for (int tx = 0; tx < a.n_tx; ++tx) {
            const float tt = tx_in_tile ? tau_rx[tx][threadIdx.x] : tfm_tau(a.tt_tx[(size_t)tx * nf + f], a.fs, a.half_t0s);
            if (CF && r0 == 0) n_tx_ok += tfm_has_path(tt);
            das_gather<2>(a.fmc + ((size_t)tx * a.n_rx + r0) * pair_len, pair_len, a.n_t, tt, tau_rx, threadIdx.x, nr,
                          [&](int, das_u32x4 v, float w) {
                              const float2 p = lerp(v, w);
                              re += p.x;
                              im += p.y;
                              if (CF) en = fmaf(p.y, p.y, fmaf(p.x, p.x, en));
                          });
        }
    }
    if (!live) return;
    a.image[f] = make_float2(re, im);
    if (CF) {
        // |S|^2 is exact in fp64 (squares of fp32 values); pairs outside the record count in N with value 0, so |S|^2 <= N E up
        // to the rounding of the fp32 sums (Cauchy-Schwarz): clamped to 1
        const double n = (double)n_tx_ok * (double)n_rx_ok;
        double c = NAN;                                               // no pair with a path
        if (n > 0.0) {
            const double s2 = (double)re * (double)re + (double)im * (double)im;
            c = en > 0.0f ? s2 / (n * (double)en) : 0.0;
            c = c > 1.0 ? 1.0 : c;
        }
        a.cf[f] = (float)c;
    }
}

template <bool CF>
__global__ __launch_bounds__(RTUS_BLOCK) void rtus_tfm_analytic_kernel(TfmaArgs a)
{
    __shared__ float tau_rx[RTUS_TFM_RX_TILE][RTUS_BLOCK];           // 64 KB, as rtus_tfm_kernel
    tfma_body<CF>(a, tau_rx, DasLerp());
}

// The carrier-aware envelope TFM (include/rtus.h, rtus_tfm_iq): the same kernel with DasIq's step between the load and the sums —
// four products for R, the lerp, one product and two transcendentals for the phasor, four products to apply it: VALU work under
// gathers that the vector-memory address path paces.
template <bool CF>
__global__ __launch_bounds__(RTUS_BLOCK) void rtus_tfm_iq_kernel(TfmaArgs a, DasIq iq)
{
    __shared__ float tau_rx[RTUS_TFM_RX_TILE][RTUS_BLOCK];           // 64 KB, as rtus_tfm_kernel
    tfma_body<CF>(a, tau_rx, iq);
}

// f_demod -> (R, nu) of DasIq; 0 <= f_demod < fs / 2 (checked by the C entries).  f_demod = 0: (1, +0, 0)
DasIq rtus_das_iq(double f_demod, double fs)
{
    const double nu = f_demod / fs, ph = 6.283185307179586476925 * nu;
    DasIq q;
    q.cs = (float)cos(ph); q.sn = (float)sin(ph); q.nu = (float)nu;
    return q;
}

hipError_t rtus_launch_tfm_analytic(const float* an, int n_tx, int n_rx, int n_t, double fs, double t0, const double* tt_tx,
                                    const double* tt_rx, int n_f, float* image, float* cf, hipStream_t s)
{
    TfmaArgs a = tfm_args<TfmaArgs>(an, n_tx, n_rx, n_t, fs, t0, tt_tx, tt_rx, n_f);
    a.image = (float2*)image; a.cf = cf;
    const dim3 grid((n_f + RTUS_BLOCK - 1) / RTUS_BLOCK), block(RTUS_BLOCK);
    if (cf) hipLaunchKernelGGL(rtus_tfm_analytic_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(rtus_tfm_analytic_kernel<false>, grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t rtus_launch_tfm_iq(const float* an, int n_tx, int n_rx, int n_t, double fs, double t0, double f_demod, const double* tt_tx,
                              const double* tt_rx, int n_f, float* image, float* cf, hipStream_t s)
{
    TfmaArgs a = tfm_args<TfmaArgs>(an, n_tx, n_rx, n_t, fs, t0, tt_tx, tt_rx, n_f);
    a.image = (float2*)image; a.cf = cf;
    const DasIq iq = rtus_das_iq(f_demod, fs);
    const dim3 grid((n_f + RTUS_BLOCK - 1) / RTUS_BLOCK), block(RTUS_BLOCK);
    if (cf) hipLaunchKernelGGL(rtus_tfm_iq_kernel<true>, grid, block, 0, s, a, iq);
    else hipLaunchKernelGGL(rtus_tfm_iq_kernel<false>, grid, block, 0, s, a, iq);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- phase-coherence TFM: vcf, scf
// rtus_tfm_analytic_kernel's delay-and-sum — the same tile, order and two statements for S, so the image has its bits — and, per
// pair, what only the gather loop can see: with PHASOR the unit phasor u = p / |p| of the interpolated sample, summed in fp32 into U;
// with SIGN the sign of Re p, summed as an integer into B.  N = T R as in the CF instantiation.  vcf = |U| / N and
// scf = 1 - sqrt(1 - (B / N)^2) in fp64 (Camacho, Parrilla & Fritsch 2009).  Definition: include/rtus.h (rtus_tfm_phase).
struct TfmpArgs {
    const float* __restrict__ fmc;       // [n_tx][n_rx][n_t][2]
    const double* __restrict__ tt_tx;    // [n_tx][n_f]
    const double* __restrict__ tt_rx;    // [n_rx][n_f]
    float2* __restrict__ image;          // [n_f]
    float* __restrict__ vcf;             // [n_f] (PHASOR only; not null there)
    float* __restrict__ scf;             // [n_f] (SIGN only, nullable)
    int2* __restrict__ counts;           // [n_f] (B, N) (SIGN only, nullable)
    int n_tx, n_rx, n_t, n_f;
    double fs, half_t0s;
};

// (tfmp_unit, the unit phasor p / |p|: rtus_das.h — the half-matrix form sums the same phasors)
template <bool PHASOR, bool SIGN>
__global__ __launch_bounds__(RTUS_BLOCK) void rtus_tfm_phase_kernel(TfmpArgs a)
{
    __shared__ float tau_rx[RTUS_TFM_RX_TILE][RTUS_BLOCK];           // 64 KB, as rtus_tfm_kernel
    const int f_raw = das_workgroup() * RTUS_BLOCK + threadIdx.x;
    const bool live = f_raw < a.n_f;
    const int f = live ? f_raw : a.n_f - 1;
    const size_t nf = (size_t)a.n_f;
    const size_t pair_len = (size_t)a.n_t * 2;                        // floats per analytic A-scan
    const bool tx_in_tile = a.tt_tx == a.tt_rx && a.n_tx == a.n_rx && a.n_rx <= RTUS_TFM_RX_TILE;
    float re = 0.0f, im = 0.0f, ure = 0.0f, uim = 0.0f;
    int sgn = 0;                                                      // B[f]: |B| <= n_tx n_rx <= 2^30
    int n_tx_ok = 0, n_rx_ok = 0;                                     // T[f], R[f]
    for (int r0 = 0; r0 < a.n_rx; r0 += RTUS_TFM_RX_TILE) {
        const int nr = min(RTUS_TFM_RX_TILE, a.n_rx - r0);
        __syncthreads();                                              // the previous tile is no longer read
        for (int r = 0; r < nr; ++r) {
            const float v = tfm_tau(a.tt_rx[(size_t)(r0 + r) * nf + f], a.fs, a.half_t0s);
            tau_rx[r][threadIdx.x] = v;
            if (PHASOR || SIGN) n_rx_ok += tfm_has_path(v);
        }
        __syncthreads();
        for (int tx = 0; tx < a.n_tx; ++tx) {
            const float tt = tx_in_tile ? tau_rx[tx][threadIdx.x] : tfm_tau(a.tt_tx[(size_t)tx * nf + f], a.fs, a.half_t0s);
            if ((PHASOR || SIGN) && r0 == 0) n_tx_ok += tfm_has_path(tt);
            das_gather<2>(a.fmc + ((size_t)tx * a.n_rx + r0) * pair_len, pair_len, a.n_t, tt, tau_rx, threadIdx.x, nr,
                          [&](int, das_u32x4 v, float w) {
                              const float2 p = das_lerp(v, w);
                              re += p.x;
                              im += p.y;
                              if (PHASOR) {
                                  const float2 u = tfmp_unit(p);
                                  ure += u.x;
                                  uim += u.y;
                              }
                              if (SIGN) sgn += (p.x > 0.0f) - (p.x < 0.0f);
                          });
        }
    }
    if (!live) return;
    a.image[f] = make_float2(re, im);
    if (PHASOR || SIGN) {
#pragma clang fp contract(off)
        const int n = n_tx_ok * n_rx_ok;                              // <= n_tx n_rx <= 2^30 (checked by the C entries)
        if (PHASOR) {
            // |U|^2 is exact to fp64 rounding (squares of fp32 values); |U| <= N up to the rounding of the fp32 sums: clamped to 1
            double c = NAN;                                           // no pair with a path
            if (n > 0) {
                c = sqrt((double)ure * (double)ure + (double)uim * (double)uim) / (double)n;
                c = c > 1.0 ? 1.0 : c;
            }
            a.vcf[f] = (float)c;
        }
        if (SIGN) {
            if (a.scf) {
                double c = NAN;
                if (n > 0) {
                    const double q = (double)sgn / (double)n;         // |q| <= 1: |B| <= N
                    c = 1.0 - sqrt(1.0 - q * q);
                }
                a.scf[f] = (float)c;
            }
            if (a.counts) a.counts[f] = make_int2(sgn, n);
        }
    }
}

hipError_t rtus_launch_tfm_phase(const float* an, int n_tx, int n_rx, int n_t, double fs, double t0, const double* tt_tx,
                                 const double* tt_rx, int n_f, float* image, float* vcf, float* scf, int* counts, hipStream_t s)
{
    TfmpArgs a = tfm_args<TfmpArgs>(an, n_tx, n_rx, n_t, fs, t0, tt_tx, tt_rx, n_f);
    a.image = (float2*)image; a.vcf = vcf; a.scf = scf; a.counts = (int2*)counts;
    const dim3 grid((n_f + RTUS_BLOCK - 1) / RTUS_BLOCK), block(RTUS_BLOCK);
    const bool sign = scf || counts;
    if (vcf && sign) hipLaunchKernelGGL((rtus_tfm_phase_kernel<true, true>), grid, block, 0, s, a);
    else if (vcf) hipLaunchKernelGGL((rtus_tfm_phase_kernel<true, false>), grid, block, 0, s, a);
    else if (sign) hipLaunchKernelGGL((rtus_tfm_phase_kernel<false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((rtus_tfm_phase_kernel<false, false>), grid, block, 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- weighted envelope TFM + sensitivity
// S[f] = sum over (tx, rx) of w_tx[tx][f] w_rx[rx][f] a[tx][rx](s), with rtus_tfm_analytic's sample positions, interpolation and edge
// rules; a leg without a path or with a non-finite weight contributes nothing.  With SENS, also P[f] = (sum over tx with a path of
// |w_tx|^2) (sum over rx with a path of |w_rx|^2), counted while the tiles are filled.  Definition: include/rtus.h (rtus_tfm_weighted).
//
// rtus_tfm_analytic_kernel's structure with a receive tile of 16 elements: the tile holds the fp32 delays AND the complex receive
// weights (16 x 256 x 12 B = 48 KiB of LDS: three workgroups per CU; 64 elements would need 192 KiB, past the CU's 160 KiB).  One
// tile is one group of sixteen gathers in flight per lane; per transmit element the tile's weighted sum goes into a partial that is
// multiplied by the transmit weight once (4 FMAs per tx and tile, not per pair).  The transmit delay and weight are re-read per tile
// (16 B per tx and focal point, against 16 x 16 B of gathers).
#define RTUS_TFMW_RX_TILE RTUS_DAS_GROUP

struct TfmwArgs {
    const float* __restrict__ fmc;       // [n_tx][n_rx][n_t][2]
    const double* __restrict__ tt_tx;    // [n_tx][n_f]
    const double* __restrict__ tt_rx;    // [n_rx][n_f]
    const float2* __restrict__ w_tx;     // [n_tx][n_f]
    const float2* __restrict__ w_rx;     // [n_rx][n_f]
    float2* __restrict__ image;          // [n_f]
    float* __restrict__ sens;            // [n_f] (read by the SENS instantiation only)
    int n_tx, n_rx, n_t, n_f;
    double fs, half_t0s;
};

// (tfmw_finite, a weight that a leg can carry: rtus_das.h)
template <bool SENS>
__global__ __launch_bounds__(RTUS_BLOCK) void rtus_tfm_weighted_kernel(TfmwArgs a)
{
    __shared__ float tau_rx[RTUS_TFMW_RX_TILE][RTUS_BLOCK];           // 16 KiB
    __shared__ float2 wr[RTUS_TFMW_RX_TILE][RTUS_BLOCK];              // 32 KiB
    const int f_raw = das_workgroup() * RTUS_BLOCK + threadIdx.x;
    const bool live = f_raw < a.n_f;
    const int f = live ? f_raw : a.n_f - 1;
    const size_t nf = (size_t)a.n_f;
    const size_t pair_len = (size_t)a.n_t * 2;                        // floats per analytic A-scan
    float re = 0.0f, im = 0.0f, ptx = 0.0f, prx = 0.0f;
    for (int r0 = 0; r0 < a.n_rx; r0 += RTUS_TFMW_RX_TILE) {
        const int nr = min(RTUS_TFMW_RX_TILE, a.n_rx - r0);
        __syncthreads();                                              // the previous tile is no longer read
        for (int r = 0; r < nr; ++r) {
            const size_t o = (size_t)(r0 + r) * nf + f;
            const float v = tfm_tau(a.tt_rx[o], a.fs, a.half_t0s);
            const float2 g = a.w_rx[o];
            const bool ok = tfm_has_path(v) && tfmw_finite(g);
            tau_rx[r][threadIdx.x] = ok ? v : RTUS_DAS_NO_PATH;       // every position of the pair is negative
            wr[r][threadIdx.x] = ok ? g : make_float2(0.0f, 0.0f);
            if (SENS && ok) prx = fmaf(g.y, g.y, fmaf(g.x, g.x, prx));
        }
        __syncthreads();
        for (int tx = 0; tx < a.n_tx; ++tx) {
            const size_t o = (size_t)tx * nf + f;
            float tt = tfm_tau(a.tt_tx[o], a.fs, a.half_t0s);
            float2 gt = a.w_tx[o];
            const bool ok = tfm_has_path(tt) && tfmw_finite(gt);
            if (!ok) { tt = RTUS_DAS_NO_PATH; gt = make_float2(0.0f, 0.0f); }
            if (SENS && r0 == 0 && ok) ptx = fmaf(gt.y, gt.y, fmaf(gt.x, gt.x, ptx));
            float pr = 0.0f, pi = 0.0f;                               // the tile's sum of w_rx a(s)
            das_gather<2>(a.fmc + ((size_t)tx * a.n_rx + r0) * pair_len, pair_len, a.n_t, tt, tau_rx, threadIdx.x, nr,
                          [&](int r, das_u32x4 v, float w) {
                              const float2 g = wr[r][threadIdx.x], p = das_lerp(v, w);
                              pr = fmaf(g.x, p.x, fmaf(-g.y, p.y, pr));
                              pi = fmaf(g.x, p.y, fmaf(g.y, p.x, pi));
                          });
            re = fmaf(gt.x, pr, fmaf(-gt.y, pi, re));
            im = fmaf(gt.x, pi, fmaf(gt.y, pr, im));
        }
    }
    if (!live) return;
    a.image[f] = make_float2(re, im);
    if (SENS) a.sens[f] = (float)((double)ptx * (double)prx);
}

hipError_t rtus_launch_tfm_weighted(const float* an, int n_tx, int n_rx, int n_t, double fs, double t0, const double* tt_tx,
                                    const double* tt_rx, const float* w_tx, const float* w_rx, int n_f, float* image, float* sens,
                                    hipStream_t s)
{
    TfmwArgs a = tfm_args<TfmwArgs>(an, n_tx, n_rx, n_t, fs, t0, tt_tx, tt_rx, n_f);
    a.w_tx = (const float2*)w_tx; a.w_rx = (const float2*)w_rx; a.image = (float2*)image; a.sens = sens;
    const dim3 grid((n_f + RTUS_BLOCK - 1) / RTUS_BLOCK), block(RTUS_BLOCK);
    if (sens) hipLaunchKernelGGL(rtus_tfm_weighted_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(rtus_tfm_weighted_kernel<false>, grid, block, 0, s, a);
    return hipGetLastError();
}
