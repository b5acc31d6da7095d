// rtus_fmcsim.hip — the forward model of the imaging side: arrivals (a time and a complex amplitude each) to the A-scans of a
// full-matrix capture, out[tx][rx][j] += a p(t_j - tau).  NOT IN THE REFERENCE: checked against tests/fmcsim_numpy.py.
// Definition, the pinned position arithmetic and the accumulation contract: include/rtus.h (rtus_fmc_sim, rtus_fmc_sim_echo).
//
//   * rtus_fmc_sim_kernel: one wave = RTUS_SIM_TILE samples of one A-scan, held in LDS (RTUS_BLOCK / RTUS_WAVE waves per
//     workgroup, which share nothing but the wavelet table: one barrier after the table is filled, none afterwards, no atomics).
//     The wavelet sits in LDS as (p[i], p[i + 1] - p[i]) in one 16-byte entry, de-interleaved by i mod oversample: the samples of
//     one arrival step through the table `oversample` entries at a time, so in this layout neighbouring lanes read neighbouring
//     entries (one conflict-free ds_read_b128 per update, whatever the oversampling).
//     64 arrivals per step: lane l loads arrival s0 + l (row reads, coalesced), forms its table position, weight, amplitude and
//     sample range once; a ballot keeps the arrivals that reach the tile; the scalar side walks the set bits in ascending order,
//     broadcasts one arrival by v_readlane, and the 64 lanes cover its samples (read-modify-write of the LDS tile: a wave's LDS
//     operations complete in order, so arrival s + 1 sees arrival s).  Every sample is therefore summed in ascending arrival order
//     whatever the launch shape.  The tile goes out in 16-byte stores.
//     LDS per workgroup: 16 (n_p + oversample) bytes of table at most, plus 4 tiles of 8 KB (complex) or 4 KB (real).
#include "rtus_device.h"

#define RTUS_SIM_TILE 1024                                   // samples of one A-scan per wave
#define RTUS_SIM_WAVES (RTUS_BLOCK / RTUS_WAVE)

struct SimArgs {
    const double* __restrict__ t1;       // scatterer form: tt_tx [n_tx][n]; echo form: t_pair [n_tx * n_rx][n]
    const double* __restrict__ t2;       // scatterer form: tt_rx [n_rx][n]; echo form: null
    const float2* __restrict__ q;        // [n] or null (scatterer form only)
    const float2* __restrict__ a1;       // scatterer form: w_tx [n_tx][n] or null; echo form: amp [n_tx * n_rx][n] or null
    const float2* __restrict__ a2;       // scatterer form: w_rx [n_rx][n] or null; echo form: null
    const float2* __restrict__ pulse;    // [n_p]
    float* __restrict__ out;             // [n_pairs][n_t] float or float2
    long long n_units;                   // n_pairs * n_tiles
    int n_rx, n, n_t, n_tiles, n_p, os, L, echo, accumulate;
    double fs, t0, centre;
};

__device__ __forceinline__ bool sim_finite(float2 v) { return fabsf(v.x) <= 3.4e38f && fabsf(v.y) <= 3.4e38f; }   // NaN fails

__device__ __forceinline__ float2 sim_cmul(float2 a, float2 b)
{
#pragma clang fp contract(off)                               // four products, each rounded; then the two sums
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// one arrival as a lane holds it
struct SimArrival {
    int base;                            // table entry of sample j: tab[base + j]
    int j_first, j_last;                 // its samples inside the record (empty: j_first > j_last)
    float w, re, im;
};

// The pinned position arithmetic (include/rtus.h): fp64, no fused multiply-add.
__device__ __forceinline__ bool sim_place(double tau, const SimArgs& a, SimArrival& r)
{
#pragma clang fp contract(off)
    const double d = ((tau - a.t0) * a.fs) * (double)a.os;   // the arrival, in table steps after the record's start
    if (!(fabs(d) < 1073741824.0)) return false;             // NaN, inf, or absurdly far: no arrival
    const double x0 = a.centre - d;                          // table position of sample 0
    const double fl = floor(x0);
    r.w = (float)(x0 - fl);                                  // (exact difference, rounded once)
    const int ip0 = (int)fl + 1;                             // padded index: entry ip holds p[ip - 1] and p[ip] - p[ip - 1], 0 <= ip <= n_p
    const int os = a.os;
    r.j_first = ip0 >= 0 ? 0 : (-ip0 + os - 1) / os;
    r.j_last = ip0 > a.n_p ? -1 : min((a.n_p - ip0) / os, a.n_t - 1);
    const int ipf = ip0 + r.j_first * os;                    // 0 <= ipf (< os where j_first > 0)
    r.base = (ipf % os) * a.L + ipf / os - r.j_first;
    return r.j_first <= r.j_last;
}

// tile <-> global, nfl floats: 16-byte accesses where the global address allows, single floats at the ends
template <bool STORE>
__device__ __forceinline__ void sim_copy(float* g, float* tile, int nfl, int lane)
{
    const int head = min((int)((16u - ((unsigned)(uintptr_t)g & 15u)) & 15u) >> 2, nfl);
    const int n4 = (nfl - head) >> 2, tail0 = head + 4 * n4;
    if (lane < head) { if (STORE) g[lane] = tile[lane]; else tile[lane] = g[lane]; }
    for (int i = lane; i < n4; i += RTUS_WAVE) {
        float* t = tile + head + 4 * i;
        float4* p = (float4*)(g + head) + i;
        if (STORE) *p = make_float4(t[0], t[1], t[2], t[3]);
        else { const float4 v = *p; t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w; }
    }
    if (lane < nfl - tail0) { if (STORE) g[tail0 + lane] = tile[tail0 + lane]; else tile[tail0 + lane] = g[tail0 + lane]; }
}

template <bool ANALYTIC>
__global__ __launch_bounds__(RTUS_BLOCK) void rtus_fmc_sim_kernel(SimArgs a)
{
    extern __shared__ float4 sim_lds[];
    constexpr int C = ANALYTIC ? 2 : 1;                      // floats per sample
    const int n_tab = a.os * a.L;
    float4* tab = sim_lds;
    for (int idx = threadIdx.x; idx < n_tab; idx += RTUS_BLOCK) {
        const int ip = (idx % a.L) * a.os + idx / a.L;       // entry ip: (p[ip - 1], p[ip] - p[ip - 1]), p[-1] = p[n_p] = 0
        float4 e = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (ip <= a.n_p) {
            const float2 lo = ip >= 1 ? a.pulse[ip - 1] : make_float2(0.0f, 0.0f);
            const float2 hi = ip < a.n_p ? a.pulse[ip] : make_float2(0.0f, 0.0f);
            e = make_float4(lo.x, lo.y, hi.x - lo.x, hi.y - lo.y);
        }
        tab[idx] = e;
    }
    __syncthreads();                                         // the only barrier: the waves share the table and nothing else
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / RTUS_WAVE), lane = threadIdx.x % RTUS_WAVE;
    const long long unit = (long long)blockIdx.x * RTUS_SIM_WAVES + wave;
    if (unit >= a.n_units) return;                           // (whole waves)
    const long long pair = unit / a.n_tiles;
    const int j0 = (int)(unit % a.n_tiles) * RTUS_SIM_TILE, j1 = min(j0 + RTUS_SIM_TILE, a.n_t) - 1;
    float* tile = (float*)(sim_lds + n_tab) + wave * (RTUS_SIM_TILE * C);
    float* g = a.out + ((size_t)pair * a.n_t + j0) * C;
    const int nfl = (j1 - j0 + 1) * C;
    if (a.accumulate) sim_copy<false>(g, tile, nfl, lane);
    else for (int i = lane; i < nfl; i += RTUS_WAVE) tile[i] = 0.0f;

    const size_t n = (size_t)a.n;
    const size_t row1 = (size_t)(a.echo ? pair : pair / a.n_rx) * n, row2 = (size_t)(pair % a.n_rx) * n;
    for (int s0 = 0; s0 < a.n; s0 += RTUS_WAVE) {
        const int s = s0 + lane;
        SimArrival r;
        bool alive = s < a.n;
        if (alive) {
            double tau = a.t1[row1 + s];
            if (a.t2) tau += a.t2[row2 + s];
            float2 amp = make_float2(1.0f, 0.0f);
            bool ok = true;
            if (a.q) { amp = a.q[s]; ok = sim_finite(amp); }
            if (a.a1) { const float2 v = a.a1[row1 + s]; ok &= sim_finite(v); amp = sim_cmul(amp, v); }
            if (a.a2) { const float2 v = a.a2[row2 + s]; ok &= sim_finite(v); amp = sim_cmul(amp, v); }
            ok &= sim_finite(amp);                           // (a product of finite factors may still overflow)
            alive = sim_place(tau, a, r) && ok && r.j_last >= j0 && r.j_first <= j1;
            r.re = amp.x; r.im = amp.y;
        }
        unsigned long long todo = __ballot(alive);
        while (todo) {                                       // ascending arrival index: the order of the sums
            const int b = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int base = __builtin_amdgcn_readlane(r.base, b);
            const int lo = max(__builtin_amdgcn_readlane(r.j_first, b), j0), hi = min(__builtin_amdgcn_readlane(r.j_last, b), j1);
            const float w = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r.w), b));
            const float are = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r.re), b));
            const float aim = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r.im), b));
            for (int j = lo + lane; j <= hi; j += RTUS_WAVE) {
                const float4 e = tab[base + j];
                const float pr = fmaf(w, e.z, e.x), pi = fmaf(w, e.w, e.y);
                if (ANALYTIC) {
                    float2* t = (float2*)tile + (j - j0);
                    float2 v = *t;
                    v.x = fmaf(-aim, pi, fmaf(are, pr, v.x));
                    v.y = fmaf(aim, pr, fmaf(are, pi, v.y));
                    *t = v;
                } else {
                    tile[j - j0] = fmaf(-aim, pi, fmaf(are, pr, tile[j - j0]));
                }
            }
        }
    }
    sim_copy<true>(g, tile, nfl, lane);
}

size_t rtus_fmc_sim_lds_bytes(int n_p, int os, int analytic)
{
    const size_t L = ((size_t)n_p + os) / os;
    return 16 * L * os + (size_t)RTUS_SIM_WAVES * RTUS_SIM_TILE * (analytic ? 8 : 4);
}

hipError_t rtus_launch_fmc_sim(const double* t1, const double* t2, const float* q, const float* a1, const float* a2, int n_tx, int n_rx,
                               int n, int echo, const float* pulse, int n_p, int centre, int os, double fs, double t0, int n_t, float* out,
                               int analytic, int accumulate, hipStream_t s)
{
    SimArgs a;
    a.t1 = t1; a.t2 = t2; a.q = (const float2*)q; a.a1 = (const float2*)a1; a.a2 = (const float2*)a2; a.pulse = (const float2*)pulse;
    a.out = out;
    a.n_rx = n_rx; a.n = n; a.n_t = n_t; a.n_tiles = (n_t + RTUS_SIM_TILE - 1) / RTUS_SIM_TILE; a.n_p = n_p; a.os = os;
    a.L = (n_p + os) / os;                                   // entries per phase: ceil((n_p + 1) / os)
    a.echo = echo; a.accumulate = accumulate;
    a.n_units = (long long)n_tx * n_rx * a.n_tiles;
    a.fs = fs; a.t0 = t0; a.centre = (double)centre;
    const dim3 grid((unsigned)((a.n_units + RTUS_SIM_WAVES - 1) / RTUS_SIM_WAVES)), block(RTUS_BLOCK);
    const size_t lds = rtus_fmc_sim_lds_bytes(n_p, os, analytic);
    if (analytic) hipLaunchKernelGGL(rtus_fmc_sim_kernel<true>, grid, block, lds, s, a);
    else hipLaunchKernelGGL(rtus_fmc_sim_kernel<false>, grid, block, lds, s, a);
    return hipGetLastError();
}
