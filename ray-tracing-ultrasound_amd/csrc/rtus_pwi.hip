// rtus_pwi.hip — plane-wave imaging (PWI): the plane wave's transmit time through planar layers, and the synthesis of any
// transmit delay law from full-matrix-capture (FMC) data.  NOT IN THE REFERENCE: checked against tests/pwi_numpy.py (itself checked
// against mpmath and a brute-force Huygens minimum).  Definitions: include/rtus.h (rtus_pw_layers, rtus_fmc_synth_tx).
//
//   * rtus_pw_layers_kernel streams the table: per angle the slowness p = sin t / c0, and per layer the vertical slowness
//     sqrt(1/c_i^2 - p^2) and the lateral drift p c_i / sqrt(1 - p^2 c_i^2), summed down to every interface — formed once per
//     workgroup in LDS.  An entry is then its layer's lookup and a few FMAs: bound by the 8-byte writes (HBM roofline).
//   * rtus_fmc_synth_tx_kernel: lanes are consecutive samples of one (rx, group of RTUS_SYNTH_VG delay laws); the loop runs over
//     tx with one accumulator per law in registers.  Each term is one range-checked 8-byte load of two neighbouring samples
//     (contiguous across the wave: one record is n_t 4 B) and one fmaf.  The records come from L2: bound by the L2 read rate.
#include "rtus_device.h"

#pragma clang fp contract(off)

// ---------------------------------------------------------------------------------------------- plane-wave times, planar layers
#define PW_LAYERS_PER_LANE 4       // focal points per lane: the per-angle set-up is shared by 1024 entries

struct PwLayersArgs {
    double zif[RTUS_MAX_LAYERS], c[RTUS_MAX_LAYERS + 1];
    int n_if, n_a, n_f;
    double xlo, xhi, za;
    const double* __restrict__ ang;
    const double* __restrict__ xf;
    const double* __restrict__ zf;
    double* __restrict__ tt;
};

__global__ void __launch_bounds__(RTUS_BLOCK) rtus_pw_layers_kernel(PwLayersArgs a)
{
    // layer i spans [ztop[i], ztop[i + 1]) (ztop[0] = z_a); W, G: the vertical time and the lateral drift accumulated above it
    __shared__ double s_w[RTUS_MAX_LAYERS + 1], s_g[RTUS_MAX_LAYERS + 1], s_W[RTUS_MAX_LAYERS + 1], s_G[RTUS_MAX_LAYERS + 1],
        s_top[RTUS_MAX_LAYERS + 1];
    __shared__ double s_p, s_xref;
    const int tid = threadIdx.x, ia = blockIdx.y;
    const double th = a.ang[ia];
    const bool aok = fabs(th) < RTUS_PI_2;                           // (NaN fails)
    double sn, cs;
    sincos(aok ? th : 0.0, &sn, &cs);
    const double p = aok ? sn / a.c[0] : NAN;
    if (tid <= a.n_if) {
        const double ci = a.c[tid], pc = p * ci;
        const bool prop = fabs(pc) < 1.0;                             // evanescent (and NaN) -> NaN
        const double r = sqrt((1.0 - pc) * (1.0 + pc));
        s_w[tid] = prop ? r / ci : NAN;                               // sqrt(1/c^2 - p^2)
        s_g[tid] = prop ? pc / r : NAN;                               // tan of the ray's angle in layer i
        s_top[tid] = tid == 0 ? a.za : a.zif[tid - 1];
    }
    if (tid == 0) { s_p = p; s_xref = sn >= 0.0 ? a.xlo : a.xhi; }
    __syncthreads();
    if (tid == 0) {
        double W = 0.0, G = 0.0;
        for (int i = 0; i <= a.n_if; ++i) {
            s_W[i] = W;
            s_G[i] = G;
            if (i < a.n_if) {
                const double h = a.zif[i] - s_top[i];
                W = fma(h, s_w[i], W);
                G = fma(h, s_g[i], G);
            }
        }
    }
    __syncthreads();
    const double pp = s_p, xref = s_xref;
    double* __restrict__ row = a.tt + (size_t)ia * a.n_f;
    const int f0 = blockIdx.x * (RTUS_BLOCK * PW_LAYERS_PER_LANE) + tid;
#pragma unroll
    for (int k = 0; k < PW_LAYERS_PER_LANE; ++k) {
        const int f = f0 + k * RTUS_BLOCK;
        if (f >= a.n_f) break;
        const double xf = a.xf[f], zf = a.zf[f];
        int L = 0;
        for (int i = 0; i < a.n_if; ++i) L += a.zif[i] < zf;          // the layer holding zf (an interface depth: the upper one)
        const double h = zf - s_top[L];
        const double t = fma(xf - xref, pp, fma(h, s_w[L], s_W[L]));
        const double xb = xf - fma(h, s_g[L], s_G[L]);                // the ray traced back to the array line
        const bool ok = zf > a.za && xb >= a.xlo && xb <= a.xhi;      // (NaN fails)
        row[f] = ok ? t : NAN;
    }
}

hipError_t rtus_launch_pw_layers(const double* z_if, const double* c, int n_if, const double* ang, int n_a, double xlo, double xhi,
                                 double za, const double* xf, const double* zf, int n_f, double* tt, hipStream_t s)
{
    PwLayersArgs a;
    for (int i = 0; i < RTUS_MAX_LAYERS; ++i) a.zif[i] = i < n_if ? z_if[i] : 0.0;
    for (int i = 0; i <= RTUS_MAX_LAYERS; ++i) a.c[i] = i <= n_if ? c[i] : 1.0;
    a.n_if = n_if; a.n_a = n_a; a.n_f = n_f;
    a.xlo = xlo; a.xhi = xhi; a.za = za;
    a.ang = ang; a.xf = xf; a.zf = zf; a.tt = tt;
    const long long per = RTUS_BLOCK * PW_LAYERS_PER_LANE, gx = ((long long)n_f + per - 1) / per;
    if (n_a > 65535 || gx > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rtus_pw_layers_kernel, dim3((unsigned)gx, (unsigned)n_a), dim3(RTUS_BLOCK), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- synthesis of a transmit law from FMC
// out[v][rx][n] = sum over tx ascending of x_{tx,rx}(n - d[v][tx] fs), linear interpolation, samples outside [0, n_t) zero.
// Per (v, tx), in fp64: sh = d fs, m = ceil(sh); the position n - sh lies between samples i = n - m and i + 1 with weight
// w = m - sh in [0, 1), rounded once to fp32; the term is fmaf(w, x[i + 1] - x[i], x[i]).  A whole-sample delay (w = 0) shifts
// the record exactly.  A law whose delay is not finite or |sh| >= 1e8 does not fire that tx (m = RTUS_SYNTH_SKIP).
#define RTUS_SYNTH_VG 8            // delay laws per workgroup (accumulators per lane)
#define RTUS_SYNTH_TXT 128         // tx per LDS tile of shifts and weights
#define RTUS_SYNTH_SKIP (-0x7fffffff)

typedef unsigned int syn_u32x2 __attribute__((ext_vector_type(2)));

// samples i and i + 1 of one record in one 8-byte load; out-of-record dwords read as zeros (the descriptor's range check).  i = -1
// (the record's first sample as the upper neighbour) loads from 0 and shifts; other negative indices are clamped out of range.
__device__ __forceinline__ float synth_term(const float* rec, int n_t, int i, float w)
{
    const __amdgpu_buffer_rsrc_t q = __builtin_amdgcn_make_buffer_rsrc((void*)rec, 0, (unsigned)n_t * 4u, 0x00020000);
    const bool lead = i == -1;
    const syn_u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(q, min((unsigned)(lead ? 0 : i), 0x3ffffff0u) * 4u, 0, 0);
    const float v0 = lead ? 0.0f : __uint_as_float(v.x), v1 = lead ? __uint_as_float(v.x) : __uint_as_float(v.y);
    return fmaf(w, v1 - v0, v0);
}

struct SynthArgs {
    const float* __restrict__ fmc;       // [n_tx][n_rx][n_t]
    const double* __restrict__ d;        // [n_v][n_tx]
    float* __restrict__ out;             // [n_v][n_rx][n_t]
    int n_tx, n_rx, n_t, n_v;
    double fs;
};

__global__ void __launch_bounds__(RTUS_BLOCK) rtus_fmc_synth_tx_kernel(SynthArgs a)
{
    __shared__ int s_m[RTUS_SYNTH_TXT][RTUS_SYNTH_VG];
    __shared__ float s_w[RTUS_SYNTH_TXT][RTUS_SYNTH_VG];
    const int tid = threadIdx.x;
    const int n = blockIdx.x * RTUS_BLOCK + tid, rx = blockIdx.y, v0 = blockIdx.z * RTUS_SYNTH_VG;
    const int nv = min(RTUS_SYNTH_VG, a.n_v - v0);
    const size_t rec_stride = (size_t)a.n_rx * a.n_t;
    float acc[RTUS_SYNTH_VG];
#pragma unroll
    for (int k = 0; k < RTUS_SYNTH_VG; ++k) acc[k] = 0.0f;
    for (int t0 = 0; t0 < a.n_tx; t0 += RTUS_SYNTH_TXT) {
        const int nt = min(RTUS_SYNTH_TXT, a.n_tx - t0);
        __syncthreads();                                              // the previous tile is no longer read
        for (int i = tid; i < RTUS_SYNTH_TXT * RTUS_SYNTH_VG; i += RTUS_BLOCK) {
            const int tx = i / RTUS_SYNTH_VG, k = i % RTUS_SYNTH_VG;
            int m = RTUS_SYNTH_SKIP;
            float w = 0.0f;
            if (tx < nt && k < nv) {
                const double sh = a.d[(size_t)(v0 + k) * a.n_tx + t0 + tx] * a.fs;
                if (fabs(sh) < 1.0e8) {                               // (NaN and infinities fail)
                    const double mc = ceil(sh);
                    m = (int)mc;
                    w = (float)(mc - sh);
                }
            }
            s_m[tx][k] = m;
            s_w[tx][k] = w;
        }
        __syncthreads();
        for (int tx = 0; tx < nt; ++tx) {
            const float* rec = a.fmc + (size_t)(t0 + tx) * rec_stride + (size_t)rx * a.n_t;   // wave-uniform
            float term[RTUS_SYNTH_VG];
#pragma unroll
            for (int k = 0; k < RTUS_SYNTH_VG; ++k) {                // all loads issued before the first is used
                const int m = s_m[tx][k];
                term[k] = m != RTUS_SYNTH_SKIP ? synth_term(rec, a.n_t, n - m, s_w[tx][k]) : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < RTUS_SYNTH_VG; ++k)
                if (s_m[tx][k] != RTUS_SYNTH_SKIP) acc[k] += term[k];  // (a skipped tx adds nothing, not even -0 + 0)
        }
    }
    if (n >= a.n_t) return;
#pragma unroll
    for (int k = 0; k < RTUS_SYNTH_VG; ++k)
        if (k < nv) a.out[((size_t)(v0 + k) * a.n_rx + rx) * a.n_t + n] = acc[k];
}

hipError_t rtus_launch_fmc_synth_tx(const float* fmc, int n_tx, int n_rx, int n_t, double fs, const double* d, int n_v, float* out,
                                    hipStream_t s)
{
    SynthArgs a;
    a.fmc = fmc; a.d = d; a.out = out;
    a.n_tx = n_tx; a.n_rx = n_rx; a.n_t = n_t; a.n_v = n_v; a.fs = fs;
    const long long gx = ((long long)n_t + RTUS_BLOCK - 1) / RTUS_BLOCK, gz = ((long long)n_v + RTUS_SYNTH_VG - 1) / RTUS_SYNTH_VG;
    if (gx > 0x7fffffffLL || n_rx > 65535 || gz > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rtus_fmc_synth_tx_kernel, dim3((unsigned)gx, (unsigned)n_rx, (unsigned)gz), dim3(RTUS_BLOCK), 0, s, a);
    return hipGetLastError();
}
