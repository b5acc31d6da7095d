// rtus_das.h — the delay-and-sum core shared by rtus_tfm_kernel, rtus_tfm_analytic_kernel, rtus_tfm_phase_kernel,
// rtus_tfm_weighted_kernel (rtus_tfm.hip), the half-matrix kernels (rtus_tfm_hmc.hip) and rtus_surface_find_kernel
// (rtus_autofocus.hip): the workgroup order, the delay clamp, the two-sample load, its interpolation and the gather loops.  A kernel keeps its tile fill, its accumulate step and its epilogue.
//
// The common shape: a lane owns one focal point; each receive element's half of the pair's sample position (in samples,
// fp32) sits in LDS for a tile of elements, lane-major (lane l reads tau[rx][l]: conflict-free); the transmit element's
// half is a register.  The A-scan of a pair is addressed through a buffer descriptor whose base is wave-uniform (SGPRs)
// and whose extent is the record: the hardware's range check returns 0 for a sample index outside [0, n_t) — no
// compare / select in the inner loop — and the two neighbouring samples come in one load.
#pragma once
#include "rtus_device.h"

// Workgroups go to the 8 XCDs round-robin, and each XCD has its own 4 MiB L2: with workgroup b on focal points
// [256 b, 256 b + 256) every XCD sees focal points from all over the image and pulls (its window of) the WHOLE FMC block
// through its L2.  XCD k takes a contiguous eighth of the workgroups' work instead — neighbouring focal points share
// their sample windows — so the FMC block is fetched about once, not once per XCD (measured: profiles/traffic_r03.json).
// A lane's sum depends on its focal point only, so the order changes no bit of the result.
__device__ __forceinline__ int das_workgroup()
{
    const int nblk = gridDim.x, per = (nblk + 7) >> 3;
    int blk = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
    if (nblk & 7) blk = blockIdx.x;                                   // (ragged grids keep the plain order)
    return blk;
}

// A leg's half of the sample position, already rounded to fp32 (once, from fp64: 1e-4 of a sample at 4096 samples), or
// the no-path value: far outside every record, and finite — the sum of two of them must not become NaN or wrap an
// integer conversion.  Every non-finite or absurd value becomes the no-path value too: +inf would pass a NaN test and
// poison the pixel through floor(inf).
#define RTUS_DAS_NO_PATH (-1.0e8f)
__device__ __forceinline__ float das_clamp(float v)
{
    return fabsf(v) < -RTUS_DAS_NO_PATH ? v : RTUS_DAS_NO_PATH;       // NaN fails the compare
}

// travel time -> half of the pair's sample position (formed in fp64, rounded once); no path, a non-finite or an absurd time ->
// RTUS_DAS_NO_PATH.  half_t0s = t0 fs / 2: each of the pair's two delays carries half of the time origin
__device__ __forceinline__ float tfm_tau(double t, double fs, double half_t0s) { return das_clamp((float)(t * fs - half_t0s)); }

__device__ __forceinline__ int tfm_has_path(float tau) { return tau > RTUS_DAS_NO_PATH; }   // a path's |tau| < 1e8

// Two neighbouring samples i, i + 1 of one A-scan (wave-uniform base) in one load: C = 1 real samples (8 bytes), C = 2
// complex samples (16 bytes).  An index outside the record (negative, huge, the sum of two no-path values) is dropped by
// the descriptor's range check and reads as zeros.
// Edges, as oracle/tfm_numpy.py defines them: a position in [n_t - 1, n_t) interpolates towards a zero sample n_t (the
// second half of the load is out of range by itself); a NEGATIVE position contributes nothing — index -1 must not wrap:
// its second sample sits at byte offset 2^32, which a range check in 32 bits would see as 0 — so negative indices (as
// unsigned: >= 2^31) are clamped to one that is out of range with every dword.  (Observed on MI355X: without the clamp the
// same load at offset 0xFFFFFFFC still returns zeros for both samples — tests/test_gpu_das_exact.py, change M1; the clamp is
// the guard that does not depend on it.)  |i| stays below 2^28 (das_clamp: each leg within +-1e8 samples), n_t <= 2^26.
typedef unsigned int das_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int das_u32x4 __attribute__((ext_vector_type(4)));
template <int C>
__device__ __forceinline__ auto das_load2(const float* rec, int n_t, int i)
{
    const __amdgpu_buffer_rsrc_t q = __builtin_amdgcn_make_buffer_rsrc((void*)rec, 0, (unsigned)n_t * (4u * C), 0x00020000);
    if constexpr (C == 1) return __builtin_amdgcn_raw_buffer_load_b64(q, min((unsigned)i, 0x3ffffff0u) * 4u, 0, 0);
    else return __builtin_amdgcn_raw_buffer_load_b128(q, min((unsigned)i, 0x1ffffff0u) * 8u, 0, 0);
}

// the loaded pair interpolated at weight w, real and imaginary parts separately
__device__ __forceinline__ float das_lerp(das_u32x2 v, float w)
{
    const float v0 = __uint_as_float(v.x), v1 = __uint_as_float(v.y);
    return fmaf(w, v1 - v0, v0);
}
__device__ __forceinline__ float2 das_lerp(das_u32x4 v, float w)
{
    const float r0 = __uint_as_float(v.x), i0 = __uint_as_float(v.y), r1 = __uint_as_float(v.z), i1 = __uint_as_float(v.w);
    return make_float2(fmaf(w, r1 - r0, r0), fmaf(w, i1 - i0, i0));
}

// The interpolation step of a kernel over the loaded pair, as an object: DasLerp is das_lerp.  DasIq is the carrier-aware step of
// rtus_tfm_iq (include/rtus.h) on complex samples: the second sample turned back by one sample of the carrier, q = a1 R with
// R = (cs, -sn) = exp(-2 pi i nu); das_lerp's form between a0 and q — the baseband signal interpolated; and the carrier put back,
// p = b exp(2 pi i nu w).  nu = f_demod / fs in cycles per sample, nu w in [0, 0.5]: the hardware's sine and cosine take their
// argument in revolutions, no range reduction and no 2 pi.  cs, sn (fp64 on the host, rounded once) and nu are wave-uniform.
// Every product is a statement of its own (no contraction: the bits do not depend on what the compiler would fuse), arranged so
// that nu = 0 — cs = 1, sn = +0, phasor (1, 0) exactly — multiplies exactly: p is then das_lerp's (a signed zero apart, which no
// running sum that starts at +0 can see).  A sample that reads as zero (sample n_t, a dropped load) stays zero under R: a position
// in [n_t - 1, n_t) gives (1 - w) a0 times the phasor, a dropped pair gives 0.
struct DasLerp {
    template <class V>
    __device__ __forceinline__ auto operator()(V v, float w) const { return das_lerp(v, w); }
};
struct DasIq {
    float cs, sn, nu;
    __device__ __forceinline__ float2 operator()(das_u32x4 v, float w) const
    {
#pragma clang fp contract(off)
        const float r0 = __uint_as_float(v.x), i0 = __uint_as_float(v.y), r1 = __uint_as_float(v.z), i1 = __uint_as_float(v.w);
        const float qr = fmaf(i1, sn, r1 * cs), qi = fmaf(-r1, sn, i1 * cs);
        const float br = fmaf(w, qr - r0, r0), bi = fmaf(w, qi - i0, i0);
        const float x = nu * w;
        const float c = __builtin_amdgcn_cosf(x), s = __builtin_amdgcn_sinf(x);
        return make_float2(fmaf(-bi, s, br * c), fmaf(br, s, bi * c));
    }
};

// One transmit element against the nr receive elements of the tile: accum(r, samples, weight) for r = 0 .. nr - 1 in
// ascending order, samples = the two at floor(tt + tau[r]) of the record rec + r * stride (rec, stride: wave-uniform, in
// floats), weight = the position's fraction.  The lane's column of the LDS tile is tau[.][lane].
//
// Sixteen receive elements per trip: 16 independent gathers in flight per lane, ALL issued before the first is consumed
// (two explicit phases: left to itself the scheduler pairs each load with its use).  An image of 256 x 256 focal points
// is 1024 waves — one per SIMD — so nothing but the wave's own loads hides the ~1 us a gather takes.  rtus_tfm_kernel
// at 64 x 64 x 2048: 4 in flight 441 us, 8: 282 us, 16: 214 us (192 us with the whole receive aperture in one tile), 32
// (two transmit elements at once): 218 us — from 16 on the vector-memory address path binds (64 scattered requests per
// wave-instruction, ~27 cycles each per CU).
#define RTUS_DAS_GROUP 16
template <int C, class Accum>
__device__ __forceinline__ void das_gather(const float* rec, size_t stride, int n_t, float tt, const float (*tau)[RTUS_BLOCK], int lane, int nr,
                                           Accum&& accum)
{
    int r = 0;
    for (; r + RTUS_DAS_GROUP <= nr; r += RTUS_DAS_GROUP) {
        decltype(das_load2<C>(rec, n_t, 0)) v[RTUS_DAS_GROUP];
        float w[RTUS_DAS_GROUP];
#pragma unroll
        for (int k = 0; k < RTUS_DAS_GROUP; ++k) {
            const float s = tt + tau[r + k][lane];
            const float fl = floorf(s);
            w[k] = s - fl;
            v[k] = das_load2<C>(rec + (size_t)(r + k) * stride, n_t, (int)fl);
        }
#pragma unroll
        for (int k = 0; k < RTUS_DAS_GROUP; ++k) accum(r + k, v[k], w[k]);
    }
    for (; r < nr; ++r) {                                             // receive elements past the last full group
        const float s = tt + tau[r][lane];
        const float fl = floorf(s);
        accum(r, das_load2<C>(rec + (size_t)r * stride, n_t, (int)fl), s - fl);
    }
}

// RTUS_DAS_GROUP gathers issued as ONE batch whose records and positions the caller walks: at(k, rec) -> the sample position of
// slot k and its record (wave-uniform), called for k ascending before any load is consumed; then accum(k, samples, weight) for k
// ascending.  For gathers that are not one row against a tile: the packed triangle of a half-matrix capture, where a group runs
// on across the ends of the (ragged) rows.  A caller with fewer than RTUS_DAS_GROUP records left fills the other slots with a
// position that the range check drops (2 RTUS_DAS_NO_PATH: the samples read as zeros, the weight is 0) and keeps them out of its
// sums: the partial group is still one batch (das_gather's tail issues its loads one by one, ~1 us each).
template <int C, class At, class Accum>
__device__ __forceinline__ void das_batch(int n_t, At&& at, Accum&& accum)
{
    decltype(das_load2<C>(nullptr, n_t, 0)) v[RTUS_DAS_GROUP];
    float w[RTUS_DAS_GROUP];
#pragma unroll
    for (int k = 0; k < RTUS_DAS_GROUP; ++k) {
        const float* rec;
        const float s = at(k, rec);
        const float fl = floorf(s);
        w[k] = s - fl;
        v[k] = das_load2<C>(rec, n_t, (int)fl);
    }
#pragma unroll
    for (int k = 0; k < RTUS_DAS_GROUP; ++k) accum(k, v[k], w[k]);
}

// What rtus_tfm_phase_kernel / rtus_tfm_weighted_kernel (rtus_tfm.hip) and their half-matrix forms (rtus_tfm_hmc.hip) share.
// p / |p| for every non-zero finite p, (0, 0) for p = 0.  |p|^2 under- or overflows in fp32 from |p| ~ 1e-19 / 1e19 on, so both
// parts are first scaled by the power of two that brings max(|re|, |im|) into [0.5, 1): exact (the smaller part may lose bits
// below 2^-126 of the larger: nothing against 0.25 <= x^2 + y^2 < 2).  One v_rsq_f32 (1 ulp), two products.  No contraction: the
// bits do not depend on what the compiler would fuse.
__device__ __forceinline__ float2 tfmp_unit(float2 p)
{
#pragma clang fp contract(off)
    const float m = fmaxf(fabsf(p.x), fabsf(p.y));
    const int e = __builtin_amdgcn_frexp_expf(m);                     // m = [0.5, 1) x 2^e (0 for m = 0)
    const float x = __builtin_amdgcn_ldexpf(p.x, -e), y = __builtin_amdgcn_ldexpf(p.y, -e);
    const float r = m > 0.0f ? __builtin_amdgcn_rsqf(fmaf(y, y, x * x)) : 0.0f;   // rsq(0) 0 would be NaN
    return make_float2(x * r, y * r);
}

// a weight that a leg of rtus_tfm_weighted can carry: both parts finite
__device__ __forceinline__ bool tfmw_finite(float2 w) { return fabsf(w.x) <= 3.4e38f && fabsf(w.y) <= 3.4e38f; }   // NaN fails
