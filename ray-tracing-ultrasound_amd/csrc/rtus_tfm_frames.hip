// rtus_tfm_frames.hip — TFM over a STACK of frames (an encoded scan: n_frames captures of one shape, imaged through the same
// travel-time tables on the same grid) in one call.  Definition, layouts and limits: include/rtus.h (rtus_tfm_frames,
// rtus_tfm_analytic_frames); figures: DESIGN.md §4 "TFM over a stack of frames".  NOT IN THE REFERENCE.
//
// Three kernels over the delay-and-sum core of rtus_das.h:
//   * rtus_fmc_pack_frames_kernel: a frame-major RF stack -> the PACKED layout packed[n_pairs][n_tx][n_rx][n_t][2], frame 2p in
//     plane 0 and frame 2p + 1 in plane 1 of pair p (the missing partner of an odd stack: +0.0).  A streaming copy;
//   * rtus_tfm_frames_kernel: rtus_tfm_analytic_kernel<false>'s structure over one pair's block of the packed stack.  The header
//     promises that S.re is rtus_tfm on the real parts and S.im rtus_tfm on the imaginary parts, bit for bit; the sums of the two
//     planes never meet — so TWO RF frames are imaged by ONE 16-byte gather per (pair of elements, focal point), where the
//     vector-memory address path, not the bytes, paces the gather (rtus_das.h);
//   * rtus_tfm_analytic_frames_kernel / rtus_tfm_iq_frames_kernel: rtus_tfm_analytic_kernel's / rtus_tfm_iq_kernel's loop with a
//     frame index: one call for an envelope stack, the same gathers.
// rtus_tfm.hip's kernels are not touched and nothing is shared with them but rtus_das.h: the loop is restated here (moving
// tfma_body has shifted rtus_tfm_analytic_kernel's register allocation before: see the comment above it).
//
// Workgroup order within a launch: blockIdx.x = slow * n_blk + b with n_blk = ceil(n_f / 256) workgroups per image; `slow` — the pair
// of frames (the frame, in the analytic kernels) — is the slowest-varying part, so the workgroups resident together mostly gather from
// one pair's block; b goes through das_workgroup()'s rule: with n_blk a multiple of 8, slow * n_blk is one too, so blockIdx.x and b
// are dealt to the same XCD and each XCD keeps its contiguous eighth of the focal points of EVERY pair.  A lane's sums depend on its
// focal point and its frame only: no bit depends on the order, on n_frames, on the partner in the pair or on how a stack is cut
// into launches.
#include "rtus_das.h"

#define RTUS_TFM_RX_TILE 64                                           // as rtus_tfm.hip: 64 KiB of LDS, 2 workgroups per CU

// How many pairs (analytic: frames) ONE launch takes; a longer stack is several launches on the stream, inside the one call.
// Measured (DESIGN.md §4 "TFM over a stack of frames"; 64 x 64 x 2048 samples): a small image needs several pairs per launch to fill
// the chip (256^2 focal points are 256 workgroups for 512 places: 8 or 9 images per launch are 0.92x to 0.97x a launch per image), but a
// launch must not grow with the stack: the XCDs drift apart over a long grid, the blocks of several pairs compete for the caches
// and the workgroup order stops matching the XCDs — one launch over 32 frames took 1.16x (RF) and 1.37x (analytic) the time of
// launches of 9 images at 256^2, 1.64x and 1.73x the time of a launch per image at 1024^2, where a single image is 4096 workgroups
// and fills the chip by itself.  So: about 2304 workgroups per launch, and one image per launch from 1153 workgroups on.  (A
// workgroup that walks through every pair with its delay tile kept — 64 table loads saved against 4096 gathers per lane and pair —
// was built and measured too: equal for RF pairs, 1.4x to 1.9x slower for analytic frames at 1024^2, and it needs the loop that
// rtus_tfm.hip's kernels do not have.)  -DRTUS_TFMF_PER_LAUNCH=K forces K (the experiment builds of those measurements).
#define RTUS_TFMF_LAUNCH_BLOCKS 2304
static int tfmf_per_launch(int n_slow, int n_blk)
{
#ifdef RTUS_TFMF_PER_LAUNCH
    const int m = RTUS_TFMF_PER_LAUNCH;
#else
    const int m = RTUS_TFMF_LAUNCH_BLOCKS / n_blk > 1 ? RTUS_TFMF_LAUNCH_BLOCKS / n_blk : 1;
#endif
    return m < n_slow ? m : n_slow;
}

struct TfmfArgs {
    const float* __restrict__ data;      // RF: packed [n_pairs][n_tx][n_rx][n_t][2]; analytic: [n_frames][n_tx][n_rx][n_t][2]
    const double* __restrict__ tt_tx;    // [n_tx][n_f]
    const double* __restrict__ tt_rx;    // [n_rx][n_f]
    float* __restrict__ images;          // RF: [n_frames][n_f]; analytic: [n_frames][n_f][2]
    float* __restrict__ cf;              // [n_frames][n_f] (read by the CF instantiations only)
    int n_frames, n_tx, n_rx, n_t, n_f;
    int n_blk;                           // workgroups per image: ceil(n_f / RTUS_BLOCK)
    double fs, half_t0s;
};

// -> the workgroup's block of 256 focal points within its image (das_workgroup()'s rule on n_blk); slow: which image(s)
__device__ __forceinline__ int tfmf_workgroup(int n_blk, int& slow)
{
    slow = blockIdx.x / n_blk;
    const int b = blockIdx.x - slow * n_blk, per = (n_blk + 7) >> 3;
    return (n_blk & 7) ? b : (b & 7) * per + (b >> 3);                // (ragged grids keep the plain order)
}

// ---------------------------------------------------------------------------------------------- pack
// packed[p][j][c] = stack[2 p + c][j], j over the n = n_tx n_rx n_t samples of a frame; plane 1 of the last pair of an odd stack is
// +0.0.  V = 4: four samples per lane — two 16-byte loads, two 16-byte stores, a wave reads 1 KiB of each frame and writes 2 KiB
// contiguous — when n is a multiple of 4 and both pointers are 16-byte aligned (every frame then starts aligned); V = 1 otherwise:
// 4-byte loads, 8-byte stores, still contiguous per wave.  blockIdx.y strides over the pairs, blockIdx.x over a frame.
template <int V>
__global__ __launch_bounds__(RTUS_BLOCK) void rtus_fmc_pack_frames_kernel(const float* __restrict__ stack, int n_frames, size_t n,
                                                                          float* __restrict__ packed)
{
    const int n_pairs = (n_frames + 1) >> 1;
    const size_t m = n / V, step = (size_t)gridDim.x * RTUS_BLOCK;
    for (int p = blockIdx.y; p < n_pairs; p += gridDim.y) {
        const float* f0 = stack + (size_t)(2 * p) * n;
        const bool two = 2 * p + 1 < n_frames;
        const float* f1 = f0 + n;                                     // (not read when the partner is absent)
        float* out = packed + (size_t)p * n * 2;
        for (size_t j = (size_t)blockIdx.x * RTUS_BLOCK + threadIdx.x; j < m; j += step) {
            if constexpr (V == 4) {
                const float4 a = ((const float4*)f0)[j];
                const float4 b = two ? ((const float4*)f1)[j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                ((float4*)out)[2 * j] = make_float4(a.x, b.x, a.y, b.y);
                ((float4*)out)[2 * j + 1] = make_float4(a.z, b.z, a.w, b.w);
            } else {
                ((float2*)out)[j] = make_float2(f0[j], two ? f1[j] : 0.0f);
            }
        }
    }
}

hipError_t rtus_launch_fmc_pack_frames(const float* stack, int n_frames, size_t n, float* packed, hipStream_t s)
{
    const int n_pairs = (n_frames + 1) / 2;
    const bool vec = !(n & 3) && !(((uintptr_t)stack | (uintptr_t)packed) & 15);
    const size_t m = vec ? n / 4 : n, blocks = (m + RTUS_BLOCK - 1) / RTUS_BLOCK;
    const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096), (unsigned)(n_pairs < 65535 ? n_pairs : 65535)), block(RTUS_BLOCK);
    if (vec) hipLaunchKernelGGL(rtus_fmc_pack_frames_kernel<4>, grid, block, 0, s, stack, n_frames, n, packed);
    else hipLaunchKernelGGL(rtus_fmc_pack_frames_kernel<1>, grid, block, 0, s, stack, n_frames, n, packed);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- RF pairs
// images[2 p][f] = the sum over (tx, rx) of plane 0 of pair p at rtus_tfm's sample position, images[2 p + 1][f] of plane 1: rtus_tfm's
// arithmetic, edge rules and order on each plane (das_lerp on a 16-byte load is das_lerp on the 8-byte loads of its two planes).
__global__ __launch_bounds__(RTUS_BLOCK) void rtus_tfm_frames_kernel(TfmfArgs a)
{
    __shared__ float tau_rx[RTUS_TFM_RX_TILE][RTUS_BLOCK];           // 64 KB, as rtus_tfm_kernel
    int p;                                                            // the pair: frames 2 p and 2 p + 1
    const int f_raw = tfmf_workgroup(a.n_blk, p) * RTUS_BLOCK + threadIdx.x;
    const bool live = f_raw < a.n_f;
    const int f = live ? f_raw : a.n_f - 1;
    const size_t nf = (size_t)a.n_f;
    const size_t rec_len = (size_t)a.n_t * 2;                         // floats per record of a pair: two planes, interleaved
    const float* block = a.data + (size_t)p * ((size_t)a.n_tx * (size_t)a.n_rx * rec_len);
    const bool tx_in_tile = a.tt_tx == a.tt_rx && a.n_tx == a.n_rx && a.n_rx <= RTUS_TFM_RX_TILE;
    float re = 0.0f, im = 0.0f;
    for (int r0 = 0; r0 < a.n_rx; r0 += RTUS_TFM_RX_TILE) {
        const int nr = min(RTUS_TFM_RX_TILE, a.n_rx - r0);
        __syncthreads();                                              // the previous tile is no longer read
        for (int r = 0; r < nr; ++r) tau_rx[r][threadIdx.x] = tfm_tau(a.tt_rx[(size_t)(r0 + r) * nf + f], a.fs, a.half_t0s);
        __syncthreads();
        for (int tx = 0; tx < a.n_tx; ++tx) {
            const float tt = tx_in_tile ? tau_rx[tx][threadIdx.x] : tfm_tau(a.tt_tx[(size_t)tx * nf + f], a.fs, a.half_t0s);
            das_gather<2>(block + ((size_t)tx * a.n_rx + r0) * rec_len, rec_len, a.n_t, tt, tau_rx, threadIdx.x, nr,
                          [&](int, das_u32x4 v, float w) {
                              const float2 q = das_lerp(v, w);
                              re += q.x;
                              im += q.y;
                          });
        }
    }
    if (!live) return;
    a.images[(size_t)(2 * p) * nf + f] = re;
    if (2 * p + 1 < a.n_frames) a.images[(size_t)(2 * p + 1) * nf + f] = im;   // (an odd stack's last pair has one frame)
}

// workgroups of one launch over `n_slow` images (pairs): the C entries refuse a call whose count does not fit a grid
long long rtus_tfm_frames_blocks(int n_slow, int n_f) { return (long long)n_slow * (((long long)n_f + RTUS_BLOCK - 1) / RTUS_BLOCK); }

// n_slow: the pairs (analytic: frames) of the call -> the arguments and the grid
static TfmfArgs tfmf_args(const float* data, int n_slow, int n_frames, int n_tx, int n_rx, int n_t, double fs, double t0, const double* tt_tx,
                          const double* tt_rx, int n_f, float* images, float* cf, dim3& grid)
{
    TfmfArgs a;
    a.data = data; a.tt_tx = tt_tx; a.tt_rx = tt_rx; a.images = images; a.cf = cf;
    a.n_frames = n_frames; a.n_tx = n_tx; a.n_rx = n_rx; a.n_t = n_t; a.n_f = n_f;
    a.n_blk = (int)rtus_tfm_frames_blocks(1, n_f);
    a.fs = fs; a.half_t0s = 0.5 * t0 * fs;
    grid = dim3((unsigned)rtus_tfm_frames_blocks(n_slow, n_f));
    return a;
}

hipError_t rtus_launch_tfm_frames(const float* packed, int n_frames, int n_tx, int n_rx, int n_t, double fs, double t0,
                                  const double* tt_tx, const double* tt_rx, int n_f, float* images, hipStream_t s)
{
    const int n_pairs = (n_frames + 1) / 2, m = tfmf_per_launch(n_pairs, (int)rtus_tfm_frames_blocks(1, n_f));
    const size_t block_len = (size_t)n_tx * n_rx * n_t * 2;
    for (int p0 = 0; p0 < n_pairs; p0 += m) {                         // pairs [p0, p0 + m): frames 2 p0 .. of the stack
        const int frames = n_frames - 2 * p0 < 2 * m ? n_frames - 2 * p0 : 2 * m;
        dim3 grid;
        const TfmfArgs a = tfmf_args(packed + (size_t)p0 * block_len, (frames + 1) / 2, frames, n_tx, n_rx, n_t, fs, t0, tt_tx, tt_rx, n_f,
                                     images + (size_t)(2 * p0) * n_f, nullptr, grid);
        hipLaunchKernelGGL(rtus_tfm_frames_kernel, grid, dim3(RTUS_BLOCK), 0, s, a);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- analytic frames
// rtus_tfm.hip's tfma_body with a frame index: the record base, image and cf are offset by the frame; everything else — the tile,
// the leg rule, the order, the two statements for S, E's two FMAs, N = T R, cf in fp64 — is that loop's, so frame k has the bits
// of rtus_tfm_analytic (Lerp = DasLerp) or rtus_tfm_iq (DasIq) on frame k alone.
template <bool CF, class Lerp>
__device__ __forceinline__ void tfmaf_body(TfmfArgs a, float (*tau_rx)[RTUS_BLOCK], Lerp lerp)
{
    int frame;
    const int f_raw = tfmf_workgroup(a.n_blk, frame) * RTUS_BLOCK + threadIdx.x;
    const bool live = f_raw < a.n_f;
    const int f = live ? f_raw : a.n_f - 1;
    const size_t nf = (size_t)a.n_f;
    const size_t pair_len = (size_t)a.n_t * 2;                        // floats per analytic A-scan
    const float* block = a.data + (size_t)frame * ((size_t)a.n_tx * (size_t)a.n_rx * pair_len);
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
            das_gather<2>(block + ((size_t)tx * a.n_rx + r0) * pair_len, pair_len, a.n_t, tt, tau_rx, threadIdx.x, nr,
                          [&](int, das_u32x4 v, float w) {
                              const float2 p = lerp(v, w);
                              re += p.x;
                              im += p.y;
                              if (CF) en = fmaf(p.y, p.y, fmaf(p.x, p.x, en));
                          });
        }
    }
    if (!live) return;
    ((float2*)a.images)[(size_t)frame * nf + f] = make_float2(re, im);
    if (CF) {
        // rtus_tfm_analytic's cf: |S|^2 exact in fp64, clamped to 1, NaN without a pair with a path
        const double n = (double)n_tx_ok * (double)n_rx_ok;
        double c = NAN;
        if (n > 0.0) {
            const double s2 = (double)re * (double)re + (double)im * (double)im;
            c = en > 0.0f ? s2 / (n * (double)en) : 0.0;
            c = c > 1.0 ? 1.0 : c;
        }
        a.cf[(size_t)frame * nf + f] = (float)c;
    }
}

template <bool CF>
__global__ __launch_bounds__(RTUS_BLOCK) void rtus_tfm_analytic_frames_kernel(TfmfArgs a)
{
    __shared__ float tau_rx[RTUS_TFM_RX_TILE][RTUS_BLOCK];           // 64 KB, as rtus_tfm_kernel
    tfmaf_body<CF>(a, tau_rx, DasLerp());
}

template <bool CF>
__global__ __launch_bounds__(RTUS_BLOCK) void rtus_tfm_iq_frames_kernel(TfmfArgs a, DasIq iq)
{
    __shared__ float tau_rx[RTUS_TFM_RX_TILE][RTUS_BLOCK];           // 64 KB, as rtus_tfm_kernel
    tfmaf_body<CF>(a, tau_rx, iq);
}

DasIq rtus_das_iq(double f_demod, double fs);                         // rtus_tfm.hip

// f_demod == 0: the linear instantiation (rtus_tfm_analytic's kernel body); f_demod > 0: rtus_tfm_iq's
hipError_t rtus_launch_tfm_analytic_frames(const float* an, int n_frames, int n_tx, int n_rx, int n_t, double fs, double t0, double f_demod,
                                           const double* tt_tx, const double* tt_rx, int n_f, float* images, float* cf, hipStream_t s)
{
    const dim3 block(RTUS_BLOCK);
    const int m = tfmf_per_launch(n_frames, (int)rtus_tfm_frames_blocks(1, n_f));
    const size_t block_len = (size_t)n_tx * n_rx * n_t * 2;
    const DasIq iq = rtus_das_iq(f_demod, fs);
    for (int k0 = 0; k0 < n_frames; k0 += m) {                        // frames [k0, k0 + m)
        const int frames = n_frames - k0 < m ? n_frames - k0 : m;
        dim3 grid;
        const TfmfArgs a = tfmf_args(an + (size_t)k0 * block_len, frames, frames, n_tx, n_rx, n_t, fs, t0, tt_tx, tt_rx, n_f,
                                     images + (size_t)k0 * n_f * 2, cf ? cf + (size_t)k0 * n_f : nullptr, grid);
        if (f_demod == 0.0) {
            if (cf) hipLaunchKernelGGL(rtus_tfm_analytic_frames_kernel<true>, grid, block, 0, s, a);
            else hipLaunchKernelGGL(rtus_tfm_analytic_frames_kernel<false>, grid, block, 0, s, a);
        } else {
            if (cf) hipLaunchKernelGGL(rtus_tfm_iq_frames_kernel<true>, grid, block, 0, s, a, iq);
            else hipLaunchKernelGGL(rtus_tfm_iq_frames_kernel<false>, grid, block, 0, s, a, iq);
        }
    }
    return hipGetLastError();
}
