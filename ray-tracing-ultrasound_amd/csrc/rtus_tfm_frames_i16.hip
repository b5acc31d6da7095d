// rtus_tfm_frames_i16.hip — TFM over a stack of INT16 frames (what an array controller delivers), four frames per 16-byte gather.
// Definition, layouts and limits: include/rtus.h (rtus_tfm_frames_i16); figures: DESIGN.md §4 "TFM over int16 frame stacks".
// NOT IN THE REFERENCE.
//
// Two kernels over the delay-and-sum core of rtus_das.h:
//   * rtus_fmc_pack_frames_i16_kernel: a frame-major int16 stack -> the PACKED layout packed[n_quads][n_tx][n_rx][n_t][4] int16, frame
//     4 q + c in plane c of quad q (the planes of the absent frames of the last quad: 0).  A streaming interleave;
//   * rtus_tfm_frames_i16_kernel: rtus_tfm_frames_kernel's structure over one quad's block.  Four int16 frames stored
//     sample-interleaved are 8 bytes per sample position — the record shape das_load2<2> and das_gather<2> address for a pair of
//     float frames: the extent n_t * 8 bytes and the 8-byte position stride are the same, the pointer type is a cast.  So ONE 16-byte
//     gather brings two neighbouring samples of FOUR frames.  The accumulate step sign-extends the eight halves, converts them to
//     float32 (exact) and forms das_lerp's fmaf(w, b - a, a) per plane into that plane's own sum: frame k has the bits of rtus_tfm on
//     the frame converted to float32.
// rtus_tfm_frames.hip's kernels are not touched; the workgroup order (tfmf_workgroup) is restated here, the workgroup count
// (rtus_tfm_frames_blocks) is that file's host function.
#include "rtus_das.h"

#define RTUS_TFM_RX_TILE 64                                           // as rtus_tfm.hip: 64 KiB of LDS, 2 workgroups per CU

long long rtus_tfm_frames_blocks(int n_slow, int n_f);                // rtus_tfm_frames.hip

// How many quads ONE launch takes: rtus_tfm_frames.hip's rule (about 2304 workgroups per launch, one quad per launch from 1153
// workgroups per image on), measured again for quads (DESIGN.md §4 "TFM over int16 frame stacks").
// -DRTUS_TFMF_I16_PER_LAUNCH=K forces K (the experiment builds of that measurement).
#define RTUS_TFMF_I16_LAUNCH_BLOCKS 2304
static int tfmf_i16_per_launch(int n_quads, int n_blk)
{
#ifdef RTUS_TFMF_I16_PER_LAUNCH
    const int m = RTUS_TFMF_I16_PER_LAUNCH;
#else
    const int m = RTUS_TFMF_I16_LAUNCH_BLOCKS / n_blk > 1 ? RTUS_TFMF_I16_LAUNCH_BLOCKS / n_blk : 1;
#endif
    return m < n_quads ? m : n_quads;
}

struct TfmfI16Args {
    const short* __restrict__ data;      // packed [n_quads][n_tx][n_rx][n_t][4]
    const double* __restrict__ tt_tx;    // [n_tx][n_f]
    const double* __restrict__ tt_rx;    // [n_rx][n_f]
    float* __restrict__ images;          // [n_frames][n_f]
    int n_frames, n_tx, n_rx, n_t, n_f;
    int n_blk;                           // workgroups per image: ceil(n_f / RTUS_BLOCK)
    double fs, half_t0s;
};

// rtus_tfm_frames.hip's tfmf_workgroup: -> the workgroup's block of 256 focal points within its images; slow: which quad
__device__ __forceinline__ int tfmf_i16_workgroup(int n_blk, int& slow)
{
    slow = blockIdx.x / n_blk;
    const int b = blockIdx.x - slow * n_blk, per = (n_blk + 7) >> 3;
    return (n_blk & 7) ? b : (b & 7) * per + (b >> 3);                // (ragged grids keep the plain order)
}

// ---------------------------------------------------------------------------------------------- pack
// packed[q][j][c] = stack[4 q + c][j], j over the n = n_tx n_rx n_t samples of a frame; the planes of absent frames are 0.
// V = 8: eight samples per lane — one 16-byte load from each frame, four 16-byte stores, a wave reads 1 KiB of each frame and writes
// 4 KiB contiguous — when n is a multiple of 8 and both pointers are 16-byte aligned (every frame then starts aligned); V = 1
// otherwise: 2-byte loads, 8-byte stores, still contiguous per wave.  blockIdx.y strides over the quads, blockIdx.x over a frame.
template <int V>
__global__ __launch_bounds__(RTUS_BLOCK) void rtus_fmc_pack_frames_i16_kernel(const short* __restrict__ stack, int n_frames, size_t n,
                                                                              short* __restrict__ packed)
{
    const int n_quads = (n_frames + 3) >> 2;
    const size_t m = n / V, step = (size_t)gridDim.x * RTUS_BLOCK;
    for (int q = blockIdx.y; q < n_quads; q += gridDim.y) {
        const short* f0 = stack + (size_t)(4 * q) * n;
        const int have = min(4, n_frames - 4 * q);                    // frames of this quad: planes have .. 3 are not read
        short* out = packed + (size_t)q * n * 4;
        for (size_t j = (size_t)blockIdx.x * RTUS_BLOCK + threadIdx.x; j < m; j += step) {
            if constexpr (V == 8) {
                const das_u32x4 zero = {0u, 0u, 0u, 0u};
                const das_u32x4 a = ((const das_u32x4*)f0)[j];
                const das_u32x4 b = have > 1 ? ((const das_u32x4*)(f0 + n))[j] : zero;
                const das_u32x4 c = have > 2 ? ((const das_u32x4*)(f0 + 2 * n))[j] : zero;
                const das_u32x4 d = have > 3 ? ((const das_u32x4*)(f0 + 3 * n))[j] : zero;
                das_u32x4* o = (das_u32x4*)out + 4 * j;               // eight positions of 8 bytes
#pragma unroll
                for (int k = 0; k < 4; ++k) {                         // dword k of each frame: positions 2 k (low halves), 2 k + 1
                    das_u32x4 v;
                    v.x = (a[k] & 0xffffu) | (b[k] << 16);
                    v.y = (c[k] & 0xffffu) | (d[k] << 16);
                    v.z = (a[k] >> 16) | (b[k] & 0xffff0000u);
                    v.w = (c[k] >> 16) | (d[k] & 0xffff0000u);
                    o[k] = v;
                }
            } else {
                const unsigned a = (unsigned short)f0[j];
                const unsigned b = have > 1 ? (unsigned short)f0[n + j] : 0u;
                const unsigned c = have > 2 ? (unsigned short)f0[2 * n + j] : 0u;
                const unsigned d = have > 3 ? (unsigned short)f0[3 * n + j] : 0u;
                das_u32x2 v;
                v.x = a | (b << 16);
                v.y = c | (d << 16);
                ((das_u32x2*)out)[j] = v;
            }
        }
    }
}

hipError_t rtus_launch_fmc_pack_frames_i16(const short* stack, int n_frames, size_t n, short* packed, hipStream_t s)
{
    const int n_quads = (n_frames + 3) / 4;
    const bool vec = !(n & 7) && !(((uintptr_t)stack | (uintptr_t)packed) & 15);
    const size_t m = vec ? n / 8 : n, blocks = (m + RTUS_BLOCK - 1) / RTUS_BLOCK;
    const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096), (unsigned)(n_quads < 65535 ? n_quads : 65535)), block(RTUS_BLOCK);
    if (vec) hipLaunchKernelGGL(rtus_fmc_pack_frames_i16_kernel<8>, grid, block, 0, s, stack, n_frames, n, packed);
    else hipLaunchKernelGGL(rtus_fmc_pack_frames_i16_kernel<1>, grid, block, 0, s, stack, n_frames, n, packed);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- int16 quads
// A dword of the load holds two planes of one sample: the low half the even plane, the high half the odd one, both signed.
__device__ __forceinline__ float i16_lo(unsigned v) { return (float)(int)(short)(v & 0xffffu); }
__device__ __forceinline__ float i16_hi(unsigned v) { return (float)((int)v >> 16); }

// images[4 q + c][f] = the sum over (tx, rx) of plane c of quad q at rtus_tfm's sample position: rtus_tfm's arithmetic, edge rules
// and order on each plane (a dropped load reads as zeros: (float)0 = +0.0, as the float kernels' dropped loads).
__global__ __launch_bounds__(RTUS_BLOCK) void rtus_tfm_frames_i16_kernel(TfmfI16Args a)
{
    __shared__ float tau_rx[RTUS_TFM_RX_TILE][RTUS_BLOCK];           // 64 KB, as rtus_tfm_kernel
    int q;                                                            // the quad: frames 4 q .. 4 q + 3
    const int f_raw = tfmf_i16_workgroup(a.n_blk, q) * RTUS_BLOCK + threadIdx.x;
    const bool live = f_raw < a.n_f;
    const int f = live ? f_raw : a.n_f - 1;
    const size_t nf = (size_t)a.n_f;
    const size_t rec_len = (size_t)a.n_t * 2;                         // a quad's record in das_gather's unit (4 bytes): n_t * 8 bytes
    const float* block = (const float*)a.data + (size_t)q * ((size_t)a.n_tx * (size_t)a.n_rx * rec_len);
    const bool tx_in_tile = a.tt_tx == a.tt_rx && a.n_tx == a.n_rx && a.n_rx <= RTUS_TFM_RX_TILE;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    for (int r0 = 0; r0 < a.n_rx; r0 += RTUS_TFM_RX_TILE) {
        const int nr = min(RTUS_TFM_RX_TILE, a.n_rx - r0);
        __syncthreads();                                              // the previous tile is no longer read
        for (int r = 0; r < nr; ++r) tau_rx[r][threadIdx.x] = tfm_tau(a.tt_rx[(size_t)(r0 + r) * nf + f], a.fs, a.half_t0s);
        __syncthreads();
        for (int tx = 0; tx < a.n_tx; ++tx) {
            const float tt = tx_in_tile ? tau_rx[tx][threadIdx.x] : tfm_tau(a.tt_tx[(size_t)tx * nf + f], a.fs, a.half_t0s);
            das_gather<2>(block + ((size_t)tx * a.n_rx + r0) * rec_len, rec_len, a.n_t, tt, tau_rx, threadIdx.x, nr,
                          [&](int, das_u32x4 v, float w) {
                              const float a0 = i16_lo(v.x), a1 = i16_hi(v.x), a2 = i16_lo(v.y), a3 = i16_hi(v.y);
                              const float b0 = i16_lo(v.z), b1 = i16_hi(v.z), b2 = i16_lo(v.w), b3 = i16_hi(v.w);
                              s0 += fmaf(w, b0 - a0, a0);
                              s1 += fmaf(w, b1 - a1, a1);
                              s2 += fmaf(w, b2 - a2, a2);
                              s3 += fmaf(w, b3 - a3, a3);
                          });
        }
    }
    if (!live) return;
    const int have = a.n_frames - 4 * q;                              // (the last quad of a ragged stack has fewer than four frames)
    float* img = a.images + (size_t)(4 * q) * nf + f;
    img[0] = s0;
    if (have > 1) img[nf] = s1;
    if (have > 2) img[2 * nf] = s2;
    if (have > 3) img[3 * nf] = s3;
}

hipError_t rtus_launch_tfm_frames_i16(const short* packed, int n_frames, int n_tx, int n_rx, int n_t, double fs, double t0,
                                      const double* tt_tx, const double* tt_rx, int n_f, float* images, hipStream_t s)
{
    const int n_blk = (int)rtus_tfm_frames_blocks(1, n_f);
    const int n_quads = (n_frames + 3) / 4, m = tfmf_i16_per_launch(n_quads, n_blk);
    const size_t block_len = (size_t)n_tx * n_rx * n_t * 4;           // int16 values per quad
    for (int q0 = 0; q0 < n_quads; q0 += m) {                         // quads [q0, q0 + m): frames 4 q0 .. of the stack
        const int frames = n_frames - 4 * q0 < 4 * m ? n_frames - 4 * q0 : 4 * m;
        TfmfI16Args a;
        a.data = packed + (size_t)q0 * block_len; a.tt_tx = tt_tx; a.tt_rx = tt_rx; a.images = images + (size_t)(4 * q0) * n_f;
        a.n_frames = frames; a.n_tx = n_tx; a.n_rx = n_rx; a.n_t = n_t; a.n_f = n_f;
        a.n_blk = n_blk;
        a.fs = fs; a.half_t0s = 0.5 * t0 * fs;
        const dim3 grid((unsigned)rtus_tfm_frames_blocks((frames + 3) / 4, n_f));
        hipLaunchKernelGGL(rtus_tfm_frames_i16_kernel, grid, dim3(RTUS_BLOCK), 0, s, a);
    }
    return hipGetLastError();
}
