// rtus_tfm_envelope_frames.hip — the streaming step behind rtus_tfm_envelope_frames_hmc (include/rtus.h; DESIGN.md §4 "Envelope TFM
// over half-matrix frame stacks"): the images of a stack as two sets of planes, or as interleaved complex values, -> what the caller
// asked for.  NOT IN THE REFERENCE.
//   PLANES, !MAG: re [n], im [n]        -> out [n][2] = (re, im)            (the split-plane route's complex images)
//   PLANES,  MAG: re [n], im [n]        -> out [n]    = |(re, im)|          (its magnitude images)
//  !PLANES,  MAG: re = z [n][2]         -> out [n]    = |z|                 (the complex route's magnitude images)
// n = n_frames n_f values, the frames' rows one after the other.  The magnitude is the header's: (float) sqrt((double) re re +
// (double) im im) — the products are exact in fp64 (24 x 24 bits), the sum rounds once, the fp64 sqrt is the compiler's correctly
// rounded sequence (the one HmcPhase::finish and rtus_trig.h's rtus_sqrt rest on), the conversion rounds once.
// V = 4: four values per lane with 16-byte loads and stores, when every pointer is 16-byte aligned; the n mod 4 values left are
// taken one by one by the first lanes of workgroup 0.  V = 1: 4- and 8-byte accesses, still contiguous per wave.  No LDS.
#include "rtus_das.h"

__device__ __forceinline__ float env_mag(float re, float im)
{
#pragma clang fp contract(off)
    const double r = (double)re, i = (double)im;
    return (float)sqrt(r * r + i * i);
}

template <bool PLANES, bool MAG>
__device__ __forceinline__ void env_one(const float* __restrict__ re, const float* __restrict__ im, size_t j, float* __restrict__ out)
{
    float x, y;
    if constexpr (PLANES) { x = re[j]; y = im[j]; }
    else { const float2 z = ((const float2*)re)[j]; x = z.x; y = z.y; }
    if constexpr (MAG) out[j] = env_mag(x, y);
    else ((float2*)out)[j] = make_float2(x, y);
}

template <bool PLANES, bool MAG, int V>
__global__ __launch_bounds__(RTUS_BLOCK) void rtus_envelope_combine_kernel(const float* __restrict__ re, const float* __restrict__ im,
                                                                           size_t n, float* __restrict__ out)
{
    static_assert(PLANES || MAG, "interleaved in, interleaved out is a copy");
    const size_t m = n / V, step = (size_t)gridDim.x * RTUS_BLOCK;
    for (size_t j = (size_t)blockIdx.x * RTUS_BLOCK + threadIdx.x; j < m; j += step) {
        if constexpr (V == 4) {
            float4 a, b;                                              // a: the four real parts, b: the imaginary parts
            if constexpr (PLANES) {
                a = ((const float4*)re)[j];
                b = ((const float4*)im)[j];
            } else {
                const float4 u = ((const float4*)re)[2 * j], v = ((const float4*)re)[2 * j + 1];
                a = make_float4(u.x, u.z, v.x, v.z);
                b = make_float4(u.y, u.w, v.y, v.w);
            }
            if constexpr (MAG) {
                ((float4*)out)[j] = make_float4(env_mag(a.x, b.x), env_mag(a.y, b.y), env_mag(a.z, b.z), env_mag(a.w, b.w));
            } else {
                ((float4*)out)[2 * j] = make_float4(a.x, b.x, a.y, b.y);
                ((float4*)out)[2 * j + 1] = make_float4(a.z, b.z, a.w, b.w);
            }
        } else {
            env_one<PLANES, MAG>(re, im, j, out);
        }
    }
    if constexpr (V == 4) {                                           // the tail: values [4 m, n)
        const size_t j = 4 * m + threadIdx.x;
        if (blockIdx.x == 0 && j < n) env_one<PLANES, MAG>(re, im, j, out);
    }
}

// re, im: the planes (im null: re holds interleaved complex values, and mag must be set); out: [n][2] (8-byte aligned), or [n] with
// mag; it must not overlap the inputs.
hipError_t rtus_launch_envelope_combine(const float* re, const float* im, size_t n, bool mag, float* out, hipStream_t s)
{
    const bool vec = !(((uintptr_t)re | (uintptr_t)im | (uintptr_t)out) & 15);
    const size_t m = vec ? n / 4 : n, blocks = (m + RTUS_BLOCK - 1) / RTUS_BLOCK;
    const dim3 grid((unsigned)(blocks < 1 ? 1 : blocks < 8192 ? blocks : 8192)), block(RTUS_BLOCK);
    if (!im) {
        if (vec) hipLaunchKernelGGL((rtus_envelope_combine_kernel<false, true, 4>), grid, block, 0, s, re, im, n, out);
        else hipLaunchKernelGGL((rtus_envelope_combine_kernel<false, true, 1>), grid, block, 0, s, re, im, n, out);
    } else if (mag) {
        if (vec) hipLaunchKernelGGL((rtus_envelope_combine_kernel<true, true, 4>), grid, block, 0, s, re, im, n, out);
        else hipLaunchKernelGGL((rtus_envelope_combine_kernel<true, true, 1>), grid, block, 0, s, re, im, n, out);
    } else {
        if (vec) hipLaunchKernelGGL((rtus_envelope_combine_kernel<true, false, 4>), grid, block, 0, s, re, im, n, out);
        else hipLaunchKernelGGL((rtus_envelope_combine_kernel<true, false, 1>), grid, block, 0, s, re, im, n, out);
    }
    return hipGetLastError();
}
