// rtus_tfm_hmc.hip — TFM and envelope TFM over a half-matrix capture (HMC): by reciprocity the A-scan of (tx i, rx j) is that of
// (tx j, rx i), so an array controller stores only the n_e (n_e + 1) / 2 records with i <= j, packed in np.triu_indices' order.
// Definition: include/rtus.h (rtus_tfm_hmc).  NOT IN THE REFERENCE; checked against tests/tfm_hmc_numpy.py.
//
// rtus_tfm_kernel's shape over the delay-and-sum core of rtus_das.h — a lane owns a focal point, das_workgroup()'s order, the
// delays of a tile of elements in LDS, sixteen gathers in flight per lane — and two things of its own:
//   * one table for both legs (tt_tx == tt_rx): s_ij == s_ji bit for bit, so ONE gather serves both and its sample counts with
//     weight 2 (1 on the diagonal): fmaf(2, a, sum) is sum + (a + a) — the pair summed first — in one rounding, because a + a is
//     exact (an a whose double overflows fp32 apart).  Two tables: two gathers per record, eight records per batch, the tile
//     holds (tau_tx, tau_rx) of its elements as a float2; the gain is the packed block alone;
//   * ragged rows: row i has n_e - i records, so a walk by rows would end almost every row in a partial group.  The columns go
//     in blocks of sixteen instead.  A row above a block meets it in exactly one batch of sixteen gathers of fixed shape —
//     rtus_tfm_kernel's instruction stream: the record and the LDS offset of slot k are compile-time steps from the row's.  Only
//     a block's own 16 x 16 triangle (136 records; 4 x 136 of 2080 at 64 elements) is ragged: it is walked as ONE run of records
//     across the row ends, unrolled, so that every (i, j), weight and LDS offset of the run is a constant too.  A block of fewer
//     than sixteen columns (n_e not a multiple of 16) takes the same walk with its state in scalar registers and a padded last
//     batch.  2112 gather requests per focal point at 64 elements (2080 and four half-empty batches), against 4096.
// A focal point's order of summation: blocks of sixteen columns ascending; in the block [c0, c0 + 16) first the rows above it
// (i < c0 ascending, j ascending through the block), then the block's own triangle (i ascending, j ascending from i).  The tile
// size decides only where a row's delays come from (LDS, or the tables for rows of earlier tiles): not a bit of the result.
// The same body over a block of a packed STACK of half-matrix frames — four int16 frames or two float32 frames per 16-byte gather
// (include/rtus.h: rtus_tfm_frames_hmc_i16, rtus_tfm_frames_hmc) — is at the end of the kernels: "stacks of half-matrix frames".
#include <type_traits>
#include "rtus_das.h"

// Elements whose delays a workgroup holds in LDS at a time: 64 KiB either way, two workgroups per CU.  One table: 64 floats per
// lane (a 64-element aperture is one tile: no delay is formed twice).  Two tables: 32 float2.  Measured (profiles/
// tfm_hmc_kernel.txt): a 64-element float2 tile (128 KiB, one workgroup per CU) is 8-11 % faster at 256^2 focal points, where
// a CU has one workgroup anyway, and 22-29 % slower at 1024^2.
#define RTUS_HMC_TILE 64
#ifndef RTUS_HMC_TILE2
#define RTUS_HMC_TILE2 32
#endif

struct HmcArgs {
    const float* __restrict__ hmc;       // [n_pairs][n_t] (analytic: [n_pairs][n_t][2]; a stack: the launch's blocks of [n_pairs][n_t][P])
    const double* __restrict__ tt_tx;    // [n_e][n_f]
    const double* __restrict__ tt_rx;    // [n_e][n_f]
    float* __restrict__ image;           // [n_f] (analytic: [n_f][2]; a stack: the launch's rows of [n_frames][n_f])
    float* __restrict__ cf;              // [n_f] (read by the CF instantiations only)
    int n_e, n_t, n_f;
    double fs, half_t0s;
};

// the sums of one focal point: C = 1 S alone (re), C = 2 S = (re, im) and with CF E (en).  A record's kind: off the diagonal, on
// it, or none (the unused slots of a partial batch: they add -0, which changes no sum, not even a -0)
enum { HMC_PAIR = 0, HMC_DIAG = 1, HMC_NONE = 2 };
template <int C, bool CF>
struct HmcSum {
    float re = 0.0f, im = 0.0f, en = 0.0f;
    // one gather for both legs: c = wgt a, wgt = 2, 1 or -0 by the record's kind
    __device__ __forceinline__ void one(float p, float wgt) { re = fmaf(wgt, p, re); }
    __device__ __forceinline__ void one(float2 p, float wgt)
    {
        re = fmaf(wgt, p.x, re);
        im = fmaf(wgt, p.y, im);
        if (CF) en = fmaf(wgt, fmaf(p.y, p.y, p.x * p.x), en);
    }
    // two gathers: c = a(s_ij) + a(s_ji), the pair first; the diagonal's second one is not counted
    static __device__ __forceinline__ float term(float p, float q, int kind) { return kind == HMC_PAIR ? p + q : kind == HMC_DIAG ? p : -0.0f; }
    __device__ __forceinline__ void two(float p, float q, int kind) { re += term(p, q, kind); }
    __device__ __forceinline__ void two(float2 p, float2 q, int kind)
    {
        re += term(p.x, q.x, kind);
        im += term(p.y, q.y, kind);
        if (CF) en += term(fmaf(p.y, p.y, p.x * p.x), fmaf(q.y, q.y, q.x * q.x), kind);
    }
};

// the delays of an element in the tile: one table a float, two tables (tau_tx, tau_rx)
template <bool TWO> struct HmcTau { typedef float type; };
template <> struct HmcTau<true> { typedef float2 type; };

// One run of records in batches of RTUS_DAS_GROUP gathers: with TRI a block's own triangle (nr rows; row r from column r on),
// else one row, of delays tr, against the block's nr columns.  Rows and columns are local to the block (tile: the tile from the
// block's first column on); rec: the first record; step: floats from a row's last record to the next row's first.  The last
// batch may be partial: its unused slots repeat the last record at a position that the range check drops, as HMC_NONE.
// The walk (r, c, rec) is wave-uniform and written as integer arithmetic and selects, not branches: a batch's LDS reads and
// gathers stay in ONE basic block, where the scheduler can issue the reads ahead.  A row of the triangle starts on the diagonal,
// where the row's delays are the column's: one LDS read per record, the row's delays kept in a register.
// NR: the block's size when it is known at compile time (a full block's triangle), else 0.  With it the walk is unrolled: every
// (r, c), kind, weight and LDS offset becomes a constant, and the triangle's batches have the fixed-shape batches' instruction
// stream (the walk itself costs ~25 scalar and 2 vector instructions per record).
// lerp: the step from a loaded pair to the interpolated sample (rtus_das.h: DasLerp, or DasIq for the carrier-aware kernels).
// Sum: the focal point's sums, one(sample, wgt) / two(sample, sample, kind) on what lerp returns (HmcSum, or HmcSum4 for a quad).
// Wts: the legs' weights beside the delays (HmcWts: rtus_tfm_hmc_weighted_kernel), or none (HmcNoWts: every other kernel, whose
// instruction stream is what it was).  With weights a slot also keeps its (r, c) — wave-uniform, constants where the walk is
// unrolled — and the sum gets one(sample, kind, row's weights, column's weights) / two(sample, sample, kind, ...): the column's
// from the tile, the row's from the tile (TRI) or from the caller (a row above the block), read when the sample is consumed.
struct HmcNoWts { static constexpr bool ON = false; };
struct HmcWts {
    static constexpr bool ON = true;
    const float4 (*tile)[RTUS_BLOCK];                                 // (w_tx.re, w_tx.im, w_rx.re, w_rx.im) of the block's columns
    float4 row;                                                       // the row's, where it is not one of the block's (!TRI)
};
template <int C, bool TWO, bool TRI, int NR = 0, class Sum, class Lerp, class Wts = HmcNoWts>
__device__ __forceinline__ void hmc_walk(Sum& sum, const float* rec, size_t len, size_t step, int n_t, int nr_,
                                         const typename HmcTau<TWO>::type (*tile)[RTUS_BLOCK], int lane, typename HmcTau<TWO>::type tr,
                                         const Lerp& lerp, const Wts& wts = Wts())
{
    constexpr int PER = TWO ? RTUS_DAS_GROUP / 2 : RTUS_DAS_GROUP;    // records per batch
    const int nr = NR ? NR : nr_;
    int left = TRI ? nr * (nr + 1) / 2 : nr;                          // (<= 2080)
    int r = 0, c = 0;
    // One batch; LAST: the run's last one, with left < PER records; past the run's last record (r, c, rec) stay on it
    auto batch = [&](auto last) {
        constexpr bool LAST = decltype(last)::value;
        int kind[PER];
        float wgt[PER];                                               // one table: 2, 1 or -0 by the record's kind
        int ri[PER], ci[PER];                                         // (with weights only)
        auto open = [&](int m) {
            if constexpr (Wts::ON) { ri[m] = r; ci[m] = c; }
            kind[m] = LAST && m >= left ? HMC_NONE : TRI && r == c ? HMC_DIAG : HMC_PAIR;
            // (in a scalar register: 1.0f's bits plus one exponent step off the diagonal, c - r >= 1 there)
            if constexpr (LAST || !TRI) wgt[m] = kind[m] == HMC_PAIR ? 2.0f : kind[m] == HMC_DIAG ? 1.0f : -0.0f;
            else wgt[m] = __int_as_float(0x3f800000 + (min(c - r, 1) << 23));
        };
        auto next = [&](int m) {
            if constexpr (LAST) {
                const bool go = m + 1 < left, wrap = TRI && c + 1 == nr;
                const int r1 = wrap ? r + 1 : r, c1 = wrap ? r1 : c + 1;
                r = go ? r1 : r;
                c = go ? c1 : c;
                rec += go ? (wrap ? len + step : len) : 0;
            } else if constexpr (TRI) {
                const int c1 = c + 1, on = min(nr - c1, 1);           // 1: the row goes on; 0: that was its last record
                r += 1 - on;                                          // (sums and a product: a compare would come back from
                c = r + on * (c1 - r);                                //  the compiler as a vector select and a read-lane)
                rec += len;
                rec += step * (size_t)(1 - on);
            } else {
                ++c;
                rec += len;
            }
        };
        if constexpr (!TWO) {
            auto at = [&](int k, const float*& q) {
                open(k);
                const float tc = tile[c][lane];
                if constexpr (TRI) tr = kind[k] == HMC_DIAG ? tc : tr;
                q = rec;
                next(k);
                return LAST && kind[k] == HMC_NONE ? 2.0f * RTUS_DAS_NO_PATH : tr + tc;
            };
            das_batch<C>(n_t, at, [&](int k, auto v, float w) {
                if constexpr (Wts::ON) sum.one(lerp(v, w), kind[k], TRI ? wts.tile[ri[k]][lane] : wts.row, wts.tile[ci[k]][lane]);
                else sum.one(lerp(v, w), wgt[k]);
            });
        } else {
            decltype(lerp(das_load2<C>(rec, n_t, 0), 0.0f)) first;
            float s_ji = 0.0f;
            auto at = [&](int k, const float*& q) {                   // slot 2 m: s_ij of the batch's record m, slot 2 m + 1: s_ji
                const int m = k >> 1;
                q = rec;
                if (k & 1) {
                    next(m);
                    return s_ji;
                }
                open(m);
                const float2 tc = tile[c][lane];
                if constexpr (TRI) {
                    tr.x = kind[m] == HMC_DIAG ? tc.x : tr.x;
                    tr.y = kind[m] == HMC_DIAG ? tc.y : tr.y;
                }
                s_ji = kind[m] == HMC_PAIR ? tc.x + tr.y : 2.0f * RTUS_DAS_NO_PATH;   // (the diagonal has one position)
                return LAST && kind[m] == HMC_NONE ? 2.0f * RTUS_DAS_NO_PATH : tr.x + tc.y;
            };
            das_batch<C>(n_t, at, [&](int k, auto v, float w) {
                if (!(k & 1)) first = lerp(v, w);
                else if constexpr (Wts::ON)
                    sum.two(first, lerp(v, w), kind[k >> 1], TRI ? wts.tile[ri[k >> 1]][lane] : wts.row, wts.tile[ci[k >> 1]][lane]);
                else sum.two(first, lerp(v, w), kind[k >> 1]);
            });
        }
    };
    if constexpr (NR != 0) {
#pragma unroll
        for (; left >= PER; left -= PER) batch(std::false_type());
    } else {
        for (; left >= PER; left -= PER) batch(std::false_type());   // (after the run's last record the walk's state is not read)
    }
    if (left) batch(std::true_type());
}

// Where a body's workgroup stands: its block of 256 focal points, its capture's first record, its sums and where they go.
// HmcImage: one capture, one image — the launch is the image (das_workgroup()).  HmcFrames (below): a quad or pair of a stack.
template <int C, bool CF>
struct HmcImage {
    typedef HmcSum<C, CF> Sum;
    static constexpr bool COUNT = false;                              // (HmcPhase: T and R are counted and handed to finish())
    __device__ __forceinline__ int block() const { return das_workgroup(); }
    __device__ __forceinline__ const float* records(const HmcArgs& a, size_t) const { return a.hmc; }
    __device__ __forceinline__ void store(const HmcArgs& a, int f, const Sum& sum) const
    {
        if constexpr (C == 1) a.image[f] = sum.re;
        else ((float2*)a.image)[f] = make_float2(sum.re, sum.im);
    }
};

template <int C, bool CF, bool TWO, class Lerp, class Where = HmcImage<C, CF>>
__device__ __forceinline__ void hmc_body(const HmcArgs& a, typename HmcTau<TWO>::type (*tile)[RTUS_BLOCK], const Lerp& lerp,
                                         const Where& where = Where())
{
    constexpr int TILE = TWO ? RTUS_HMC_TILE2 : RTUS_HMC_TILE;
    static_assert(TILE % RTUS_DAS_GROUP == 0, "a tile is a whole number of column blocks");
    typedef typename HmcTau<TWO>::type Tau;
    const int lane = threadIdx.x;
    const int f_raw = where.block() * RTUS_BLOCK + lane;
    const bool live = f_raw < a.n_f;
    const int f = live ? f_raw : a.n_f - 1;
    const size_t nf = (size_t)a.n_f, ne = (size_t)a.n_e;
    const size_t len = (size_t)a.n_t * C;                             // floats per record
    auto tau = [&](int e) -> Tau {                                    // element e's delays, from the tables
        const float t = tfm_tau(a.tt_tx[(size_t)e * nf + f], a.fs, a.half_t0s);
        if constexpr (TWO) return make_float2(t, tfm_tau(a.tt_rx[(size_t)e * nf + f], a.fs, a.half_t0s));
        else return t;
    };
    const float* records = where.records(a, len);                     // record (0, 0) of the workgroup's capture
    typename Where::Sum sum;
    constexpr bool COUNT = CF || Where::COUNT;
    int n_tx_ok = 0, n_rx_ok = 0;                                     // T[f], R[f] (COUNT only)
    for (int r0 = 0; r0 < a.n_e; r0 += TILE) {
        const int nr = min(TILE, a.n_e - r0);
        __syncthreads();                                              // the previous tile is no longer read
        for (int r = 0; r < nr; ++r) {
            const Tau v = tau(r0 + r);
            tile[r][lane] = v;
            if constexpr (COUNT && TWO) { n_tx_ok += tfm_has_path(v.x); n_rx_ok += tfm_has_path(v.y); }
            else if constexpr (COUNT) n_tx_ok += tfm_has_path(v);
        }
        __syncthreads();
        // the tile's columns in blocks of RTUS_DAS_GROUP: a row above a block meets it in ONE batch of fixed shape (the record
        // and the LDS offset of slot k are compile-time steps from the row's: rtus_tfm_kernel's instruction stream); only the
        // block's own triangle (136 records of 2080 at 64 elements: 4 x 136 in all) pays for the walk across ragged rows
        for (int cb = 0; cb < nr; cb += RTUS_DAS_GROUP) {
            const int nb = min(RTUS_DAS_GROUP, nr - cb), cg = r0 + cb;   // the block's columns, its first one
            const float* row = records + (size_t)cg * len;                // record (i, cg): p(i, cg) = i n_e - i (i + 1) / 2 + cg
            size_t down = (ne - 1) * len;                                 // from (i, cg) to (i + 1, cg): n_e - 1 - i records
            // rows of earlier tiles: their delays come from memory (a load that a gather's batch must not wait for)
            for (int i = 0; i < r0; ++i, row += down, down -= len)
                hmc_walk<C, TWO, false>(sum, row, len, 0, a.n_t, nb, tile + cb, lane, tau(i), lerp);
            // rows of this tile above the block: their delays are in the tile
            for (int i = r0; i < cg; ++i, row += down, down -= len)
                hmc_walk<C, TWO, false>(sum, row, len, 0, a.n_t, nb, tile + cb, lane, tile[i - r0][lane], lerp);
            // the block's own triangle from (cg, cg) on; a row's records to the right of the block are stepped over
            const size_t past = (ne - (size_t)(cg + nb)) * len;
            if (nb == RTUS_DAS_GROUP) hmc_walk<C, TWO, true, RTUS_DAS_GROUP>(sum, row, len, past, a.n_t, nb, tile + cb, lane, Tau(), lerp);
            else hmc_walk<C, TWO, true>(sum, row, len, past, a.n_t, nb, tile + cb, lane, Tau(), lerp);
        }
    }
    if (!live) return;
    where.store(a, f, sum);
    if constexpr (Where::COUNT) where.finish(f, sum, n_tx_ok, TWO ? n_rx_ok : n_tx_ok);
    if constexpr (CF) {
        // as rtus_tfm_analytic_kernel: |S|^2 exact in fp64, N = T R, clamped to 1
        if constexpr (!TWO) n_rx_ok = n_tx_ok;
        const double n = (double)n_tx_ok * (double)n_rx_ok;
        double c = NAN;                                               // no pair with a path
        if (n > 0.0) {
            const double s2 = (double)sum.re * (double)sum.re + (double)sum.im * (double)sum.im;
            c = sum.en > 0.0f ? s2 / (n * (double)sum.en) : 0.0;
            c = c > 1.0 ? 1.0 : c;
        }
        a.cf[f] = (float)c;
    }
}

template <bool TWO>
__global__ __launch_bounds__(RTUS_BLOCK) void rtus_tfm_hmc_kernel(HmcArgs a)
{
    __shared__ typename HmcTau<TWO>::type tile[TWO ? RTUS_HMC_TILE2 : RTUS_HMC_TILE][RTUS_BLOCK];
    hmc_body<1, false, TWO>(a, tile, DasLerp());
}

template <bool CF, bool TWO>
__global__ __launch_bounds__(RTUS_BLOCK) void rtus_tfm_analytic_hmc_kernel(HmcArgs a)
{
    __shared__ typename HmcTau<TWO>::type tile[TWO ? RTUS_HMC_TILE2 : RTUS_HMC_TILE][RTUS_BLOCK];
    hmc_body<2, CF, TWO>(a, tile, DasLerp());
}

// the carrier-aware form (include/rtus.h, rtus_tfm_iq_hmc): DasIq's step on every gathered pair, in every form of the walk; a
// padded slot reads zeros, which the step leaves zero
template <bool CF, bool TWO>
__global__ __launch_bounds__(RTUS_BLOCK) void rtus_tfm_hmc_iq_kernel(HmcArgs a, DasIq iq)
{
    __shared__ typename HmcTau<TWO>::type tile[TWO ? RTUS_HMC_TILE2 : RTUS_HMC_TILE][RTUS_BLOCK];
    hmc_body<2, CF, TWO>(a, tile, iq);
}

// ---------------------------------------------------------------------------------------------- stacks of half-matrix frames
// rtus_tfm_frames_hmc[_i16] (include/rtus.h; DESIGN.md §4 "TFM over half-matrix frame stacks"): the body above over one block of a
// packed stack, packed[n_slow][n_pairs][n_t][P] — P = 2 float32 frames (a pair) or P = 4 int16 frames (a quad) sample-interleaved,
// 8 bytes per sample position either way: the record shape hmc_body<2, ...> addresses for analytic data, len = 2 n_t floats.
// Plane c of block q is frame P q + c; every plane has its own sum, fed exactly as HmcSum<1, false> feeds its one: frame k has the
// bits of rtus_tfm_hmc on frame k as float32.  The workgroup order is rtus_tfm_frames.hip's (tfmf_workgroup, restated here).

// the sums of the four planes of a quad: HmcSum<1, false>'s statements on each
struct HmcSum4 {
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    __device__ __forceinline__ void one(float4 p, float wgt)
    {
        s0 = fmaf(wgt, p.x, s0);
        s1 = fmaf(wgt, p.y, s1);
        s2 = fmaf(wgt, p.z, s2);
        s3 = fmaf(wgt, p.w, s3);
    }
    __device__ __forceinline__ void two(float4 p, float4 q, int kind)
    {
        s0 += HmcSum<1, false>::term(p.x, q.x, kind);
        s1 += HmcSum<1, false>::term(p.y, q.y, kind);
        s2 += HmcSum<1, false>::term(p.z, q.z, kind);
        s3 += HmcSum<1, false>::term(p.w, q.w, kind);
    }
};

// rtus_tfm_frames_i16_kernel's accumulate step up to the sum, as a Lerp: a dword of the 16-byte load holds two planes of one sample
// (low half the even plane, high half the odd one, both signed); the eight halves sign-extended and converted (exact), then
// das_lerp's fmaf(w, b - a, a) per plane.  A dropped load reads as zeros: (float)0 = +0.0, as the float kernels' dropped loads.
struct DasQuadI16 {
    static __device__ __forceinline__ float lo(unsigned v) { return (float)(int)(short)(v & 0xffffu); }
    static __device__ __forceinline__ float hi(unsigned v) { return (float)((int)v >> 16); }
    __device__ __forceinline__ float4 operator()(das_u32x4 v, float w) const
    {
        const float a0 = lo(v.x), a1 = hi(v.x), a2 = lo(v.y), a3 = hi(v.y);
        const float b0 = lo(v.z), b1 = hi(v.z), b2 = lo(v.w), b3 = hi(v.w);
        return make_float4(fmaf(w, b0 - a0, a0), fmaf(w, b1 - a1, a1), fmaf(w, b2 - a2, a2), fmaf(w, b3 - a3, a3));
    }
};

// A workgroup of a launch over n_slow blocks of P frames: blockIdx.x = slow * n_blk + b, n_blk = ceil(n_f / 256) workgroups per
// image, b through das_workgroup()'s rule on n_blk.  n_frames: the frames of the launch; the rows of the absent frames of its last
// block do not exist and are not written.
template <int P>
struct HmcFrames {
    typedef std::conditional_t<P == 4, HmcSum4, HmcSum<2, false>> Sum;
    static constexpr bool COUNT = false;
    int n_frames, n_blk;
    __device__ __forceinline__ int slow() const { return blockIdx.x / n_blk; }
    __device__ __forceinline__ int block() const
    {
        const int b = blockIdx.x - slow() * n_blk, per = (n_blk + 7) >> 3;
        return (n_blk & 7) ? b : (b & 7) * per + (b >> 3);            // (ragged grids keep the plain order)
    }
    __device__ __forceinline__ const float* records(const HmcArgs& a, size_t len) const
    {
        const size_t n_pairs = (size_t)a.n_e * ((size_t)a.n_e + 1) / 2;
        return a.hmc + (size_t)slow() * (n_pairs * len);
    }
    __device__ __forceinline__ void store(const HmcArgs& a, int f, const Sum& sum) const
    {
        const size_t nf = (size_t)a.n_f;
        const int have = n_frames - P * slow();
        float* img = a.image + (size_t)(P * slow()) * nf + f;
        if constexpr (P == 4) {
            img[0] = sum.s0;
            if (have > 1) img[nf] = sum.s1;
            if (have > 2) img[2 * nf] = sum.s2;
            if (have > 3) img[3 * nf] = sum.s3;
        } else {
            img[0] = sum.re;
            if (have > 1) img[nf] = sum.im;
        }
    }
};

template <bool TWO>
__global__ __launch_bounds__(RTUS_BLOCK) void rtus_tfm_frames_hmc_i16_kernel(HmcArgs a, HmcFrames<4> frames)
{
    __shared__ typename HmcTau<TWO>::type tile[TWO ? RTUS_HMC_TILE2 : RTUS_HMC_TILE][RTUS_BLOCK];
    hmc_body<2, false, TWO>(a, tile, DasQuadI16(), frames);
}

// float32 pairs: the analytic body itself (each plane rtus_tfm_hmc of that plane) with the frames' base and epilogue
template <bool TWO>
__global__ __launch_bounds__(RTUS_BLOCK) void rtus_tfm_frames_hmc_f32_kernel(HmcArgs a, HmcFrames<2> frames)
{
    __shared__ typename HmcTau<TWO>::type tile[TWO ? RTUS_HMC_TILE2 : RTUS_HMC_TILE][RTUS_BLOCK];
    hmc_body<2, false, TWO>(a, tile, DasLerp(), frames);
}

// ---------------------------------------------------------------------------------------------- phase coherence: vcf, scf
// rtus_tfm_phase_hmc (include/rtus.h): rtus_tfm_analytic_hmc_kernel's body — the same walk and the same two statements for S, so
// the image has its bits — with rtus_tfm_phase_kernel's sums fed per record: with PHASOR the unit phasors of the record's one or two
// samples (tfmp_unit, rtus_das.h), the pair's two added first; with SIGN the signs of their real parts as an integer.  One table:
// the one sample's phasor and sign count twice off the diagonal, U = fmaf(wgt, u, U) as S.  T and R are counted while the tile is
// filled (hmc_body, Where::COUNT); vcf and scf are rtus_tfm_phase_kernel's epilogue.
// Resources (code-object metadata, gfx950): no scratch in any of the eight instantiations; LDS 64 KiB as the other half-matrix
// kernels: two workgroups per CU, two waves per SIMD, which every count below allows (<= 256).  VGPRs <PHASOR, SIGN, TWO>:
//   <0,0,0> 120   <1,0,0> 124   <0,1,0> 223   <1,1,0> 231   <0,0,1> 135   <1,0,1> 140   <0,1,1> 151   <1,1,1> 151
// (<0,0,*> are rtus_tfm_analytic_hmc_kernel<false, *>'s instruction streams; with SIGN and one table the scheduler keeps more of the
// unrolled triangle's loads in flight; <*,1,1> park one VGPR in an accumulation register, not in memory).
template <bool PHASOR, bool SIGN>
struct HmcPhaseSum {
    float re = 0.0f, im = 0.0f, ure = 0.0f, uim = 0.0f;
    int sgn = 0;                                                      // B[f]: |B| <= n_e^2 <= 2^30
    static __device__ __forceinline__ int sign(float x) { return (x > 0.0f) - (x < 0.0f); }
    __device__ __forceinline__ void one(float2 p, float wgt)
    {
        re = fmaf(wgt, p.x, re);
        im = fmaf(wgt, p.y, im);
        if (PHASOR) {
            const float2 u = tfmp_unit(p);
            ure = fmaf(wgt, u.x, ure);
            uim = fmaf(wgt, u.y, uim);
        }
        if (SIGN) sgn += (int)wgt * sign(p.x);                        // wgt: 2, 1 or -0
    }
    __device__ __forceinline__ void two(float2 p, float2 q, int kind)
    {
        re += HmcSum<2, false>::term(p.x, q.x, kind);
        im += HmcSum<2, false>::term(p.y, q.y, kind);
        if (PHASOR) {
            const float2 u = tfmp_unit(p), v = tfmp_unit(q);
            ure += HmcSum<2, false>::term(u.x, v.x, kind);
            uim += HmcSum<2, false>::term(u.y, v.y, kind);
        }
        if (SIGN) sgn += kind == HMC_PAIR ? sign(p.x) + sign(q.x) : kind == HMC_DIAG ? sign(p.x) : 0;
    }
};

template <bool PHASOR, bool SIGN>
struct HmcPhase {
    typedef HmcPhaseSum<PHASOR, SIGN> Sum;
    static constexpr bool COUNT = PHASOR || SIGN;
    float* __restrict__ vcf;             // [n_f] (PHASOR only; not null there)
    float* __restrict__ scf;             // [n_f] (SIGN only, nullable)
    int2* __restrict__ counts;           // [n_f] (B, N) (SIGN only, nullable)
    __device__ __forceinline__ int block() const { return das_workgroup(); }
    __device__ __forceinline__ const float* records(const HmcArgs& a, size_t) const { return a.hmc; }
    __device__ __forceinline__ void store(const HmcArgs& a, int f, const Sum& sum) const { ((float2*)a.image)[f] = make_float2(sum.re, sum.im); }
    // rtus_tfm_phase_kernel's epilogue on the half matrix's sums
    __device__ __forceinline__ void finish(int f, const Sum& sum, int n_tx_ok, int n_rx_ok) const
    {
#pragma clang fp contract(off)
        const int n = n_tx_ok * n_rx_ok;                              // <= n_e^2 <= 2^30 (checked by the C entries)
        if (PHASOR) {
            double c = NAN;                                           // no pair with a path
            if (n > 0) {
                c = sqrt((double)sum.ure * (double)sum.ure + (double)sum.uim * (double)sum.uim) / (double)n;
                c = c > 1.0 ? 1.0 : c;
            }
            vcf[f] = (float)c;
        }
        if (SIGN) {
            if (scf) {
                double c = NAN;
                if (n > 0) {
                    const double q = (double)sum.sgn / (double)n;     // |q| <= 1: |B| <= N
                    c = 1.0 - sqrt(1.0 - q * q);
                }
                scf[f] = (float)c;
            }
            if (counts) counts[f] = make_int2(sum.sgn, n);
        }
    }
};

template <bool PHASOR, bool SIGN, bool TWO>
__global__ __launch_bounds__(RTUS_BLOCK) void rtus_tfm_hmc_phase_kernel(HmcArgs a, HmcPhase<PHASOR, SIGN> where)
{
    __shared__ typename HmcTau<TWO>::type tile[TWO ? RTUS_HMC_TILE2 : RTUS_HMC_TILE][RTUS_BLOCK];
    hmc_body<2, false, TWO>(a, tile, DasLerp(), where);
}

// ---------------------------------------------------------------------------------------------- weighted envelope TFM + sensitivity
// rtus_tfm_weighted_hmc (include/rtus.h): S[f] = the sum over the records of c_ii = W_ii a_ii(s_ii), c_ij = W_ij a_ij(s_ij) +
// W_ji a_ij(s_ji), W_ij = w_tx[i] w_rx[j], in rtus_tfm_hmc's order.  hmc_walk with weights (HmcWts): a record's sample meets the
// weights of its row and of its column when it is consumed.
// The tile: an element carries its delay(s) and BOTH its weights, (w_tx, w_rx) as a float4 — 20 B per element and lane with one
// delay table, 24 B with two: 5 / 6 KiB per element of the 160 KiB a CU has.  A tile must be a whole number of column blocks
// (RTUS_DAS_GROUP = 16 elements: 80 / 96 KiB); two blocks would be 160 / 192 KiB, the whole CU or more.  So the tile IS one column
// block: one workgroup per CU with two delay tables (96 KiB), and with one (80 KiB: two would need the CU's last byte).  Rows above the
// block (i < c0) take their delay and weights from memory: 24 / 32 B per row and block against 16 gathers of 16 B — at 64 elements 96
// such rows per focal point, 2.3 / 3 KiB beside 33 KiB of gathers.
// A leg has a path only if its time has one and its weight is finite.  Two delay tables: such a leg's delay becomes the no-path value
// and its weight 0, as rtus_tfm_weighted_kernel does.  One delay table: element i's ONE delay serves its transmit and its receive
// leg, which can differ (w_tx[i] finite, w_rx[i] not), so the delay stays (no path only if the time has none) and the leg's weight
// alone becomes 0: W = 0 exactly, and 0 times the finite sample adds nothing.
// Resources (code-object metadata, gfx950): no scratch, no spills.  <SENS, TWO>: <0,0> 180 VGPRs, 80 KiB LDS; <1,0> 182, 80 KiB;
// <0,1> 186, 96 KiB; <1,1> 188, 96 KiB.  One workgroup per CU — one wave per SIMD — by LDS in all four (whether the hardware places two
// 80 KiB workgroups in a CU's 160 KiB was not measured); the registers would allow two.
struct HmcwArgs {
    HmcArgs a;                           // (cf unused)
    const float2* __restrict__ w_tx;     // [n_e][n_f]
    const float2* __restrict__ w_rx;     // [n_e][n_f]
    float* __restrict__ sens;            // [n_f] (read by the SENS instantiations only)
};

// The fp32 statements of include/rtus.h (rtus_tfm_weighted_hmc), nothing contracted beyond the fmaf's written here.
struct HmcwSum {
    float re = 0.0f, im = 0.0f;
    // a b, symmetric in its operands: the products commute and so does the sum of the imaginary part's two
    static __device__ __forceinline__ float2 cmul(float2 a, float2 b)
    {
#pragma clang fp contract(off)
        const float t = a.x * b.y, u = a.y * b.x;
        return make_float2(fmaf(-a.y, b.y, a.x * b.x), t + u);
    }
    static __device__ __forceinline__ float2 times(float2 g, float2 p)   // W a(s)
    {
#pragma clang fp contract(off)
        return make_float2(fmaf(-g.y, p.y, g.x * p.x), fmaf(g.x, p.y, g.y * p.x));
    }
    static __device__ __forceinline__ float2 w_tx(float4 g) { return make_float2(g.x, g.y); }
    static __device__ __forceinline__ float2 w_rx(float4 g) { return make_float2(g.z, g.w); }
    // one gather for both legs: c = (W_ij + W_ji) a, the weights' sum first; the diagonal W_ii a; an unused slot nothing
    __device__ __forceinline__ void one(float2 p, int kind, float4 gr, float4 gc)
    {
        const float2 wij = cmul(w_tx(gr), w_rx(gc)), wji = cmul(w_tx(gc), w_rx(gr));
        float2 g;
        g.x = kind == HMC_PAIR ? wij.x + wji.x : kind == HMC_DIAG ? wij.x : 0.0f;
        g.y = kind == HMC_PAIR ? wij.y + wji.y : kind == HMC_DIAG ? wij.y : 0.0f;
        const float2 c = times(g, p);
        re += c.x;
        im += c.y;
    }
    // two gathers: c = W_ij a(s_ij) + W_ji a(s_ji), the pair first
    __device__ __forceinline__ void two(float2 p, float2 q, int kind, float4 gr, float4 gc)
    {
        const float2 c1 = times(cmul(w_tx(gr), w_rx(gc)), p), c2 = times(cmul(w_tx(gc), w_rx(gr)), q);
        re += kind == HMC_PAIR ? c1.x + c2.x : kind == HMC_DIAG ? c1.x : 0.0f;
        im += kind == HMC_PAIR ? c1.y + c2.y : kind == HMC_DIAG ? c1.y : 0.0f;
    }
};

#define RTUS_HMCW_TILE RTUS_DAS_GROUP
template <bool SENS, bool TWO>
__global__ __launch_bounds__(RTUS_BLOCK) void rtus_tfm_hmc_weighted_kernel(HmcwArgs g)
{
    typedef typename HmcTau<TWO>::type Tau;
    __shared__ Tau tile[RTUS_HMCW_TILE][RTUS_BLOCK];                  // 16 / 32 KiB
    __shared__ float4 wtile[RTUS_HMCW_TILE][RTUS_BLOCK];              // 64 KiB
    const HmcArgs& a = g.a;
    const int lane = threadIdx.x;
    const int f_raw = das_workgroup() * RTUS_BLOCK + lane;
    const bool live = f_raw < a.n_f;
    const int f = live ? f_raw : a.n_f - 1;
    const size_t nf = (size_t)a.n_f, ne = (size_t)a.n_e;
    const size_t len = (size_t)a.n_t * 2;                             // floats per record
    float ptx = 0.0f, prx = 0.0f;
    // element e's delay(s) and weights under the leg rule; sens: its share of P is counted (once per element: the tile's fill)
    auto elem = [&](int e, Tau& tau, float4& w, bool sens) {
        const size_t o = (size_t)e * nf + f;
        const float tt = tfm_tau(a.tt_tx[o], a.fs, a.half_t0s);
        const float tr = TWO ? tfm_tau(a.tt_rx[o], a.fs, a.half_t0s) : tt;
        const float2 gt = g.w_tx[o], gr = g.w_rx[o];
        const bool ok_t = tfm_has_path(tt) && tfmw_finite(gt), ok_r = tfm_has_path(tr) && tfmw_finite(gr);
        if constexpr (TWO) tau = make_float2(ok_t ? tt : RTUS_DAS_NO_PATH, ok_r ? tr : RTUS_DAS_NO_PATH);
        else tau = tt;
        w = make_float4(ok_t ? gt.x : 0.0f, ok_t ? gt.y : 0.0f, ok_r ? gr.x : 0.0f, ok_r ? gr.y : 0.0f);
        if (SENS && sens) {
            if (ok_t) ptx = fmaf(gt.y, gt.y, fmaf(gt.x, gt.x, ptx));
            if (ok_r) prx = fmaf(gr.y, gr.y, fmaf(gr.x, gr.x, prx));
        }
    };
    HmcwSum sum;
    const DasLerp lerp;
    for (int c0 = 0; c0 < a.n_e; c0 += RTUS_HMCW_TILE) {              // the tile is the column block [c0, c0 + nb)
        const int nb = min(RTUS_HMCW_TILE, a.n_e - c0);
        __syncthreads();                                              // the previous tile is no longer read
        for (int r = 0; r < nb; ++r) {
            Tau t;
            float4 w;
            elem(c0 + r, t, w, true);
            tile[r][lane] = t;
            wtile[r][lane] = w;
        }
        __syncthreads();
        const float* row = a.hmc + (size_t)c0 * len;                  // record (i, c0): p(i, c0) = i n_e - i (i + 1) / 2 + c0
        size_t down = (ne - 1) * len;                                 // from (i, c0) to (i + 1, c0): n_e - 1 - i records
        HmcWts wts = {wtile, make_float4(0.0f, 0.0f, 0.0f, 0.0f)};
        for (int i = 0; i < c0; ++i, row += down, down -= len) {      // the rows above the block: delay and weights from memory
            Tau t;
            elem(i, t, wts.row, false);
            hmc_walk<2, TWO, false>(sum, row, len, 0, a.n_t, nb, tile, lane, t, lerp, wts);
        }
        const size_t past = (ne - (size_t)(c0 + nb)) * len;           // the block's own triangle from (c0, c0) on
        if (nb == RTUS_DAS_GROUP) hmc_walk<2, TWO, true, RTUS_DAS_GROUP>(sum, row, len, past, a.n_t, nb, tile, lane, Tau(), lerp, wts);
        else hmc_walk<2, TWO, true>(sum, row, len, past, a.n_t, nb, tile, lane, Tau(), lerp, wts);
    }
    if (!live) return;
    ((float2*)a.image)[f] = make_float2(sum.re, sum.im);
    if (SENS) g.sens[f] = (float)((double)ptx * (double)prx);
}

static HmcArgs hmc_args(const float* hmc, int n_e, int n_t, double fs, double t0, const double* tt_tx, const double* tt_rx, int n_f,
                        float* image, float* cf)
{
    HmcArgs a;
    a.hmc = hmc; a.tt_tx = tt_tx; a.tt_rx = tt_rx; a.image = image; a.cf = cf;
    a.n_e = n_e; a.n_t = n_t; a.n_f = n_f;
    a.fs = fs; a.half_t0s = 0.5 * t0 * fs;
    return a;
}

hipError_t rtus_launch_tfm_hmc(const float* hmc, int n_e, int n_t, double fs, double t0, const double* tt_tx, const double* tt_rx,
                               int n_f, float* image, hipStream_t s)
{
    const HmcArgs a = hmc_args(hmc, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f, image, nullptr);
    const dim3 grid((n_f + RTUS_BLOCK - 1) / RTUS_BLOCK), block(RTUS_BLOCK);
    if (tt_tx == tt_rx) hipLaunchKernelGGL(rtus_tfm_hmc_kernel<false>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(rtus_tfm_hmc_kernel<true>, grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t rtus_launch_tfm_analytic_hmc(const float* an, int n_e, int n_t, double fs, double t0, const double* tt_tx,
                                        const double* tt_rx, int n_f, float* image, float* cf, hipStream_t s)
{
    const HmcArgs a = hmc_args(an, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f, image, cf);
    const dim3 grid((n_f + RTUS_BLOCK - 1) / RTUS_BLOCK), block(RTUS_BLOCK);
    const bool two = tt_tx != tt_rx;
    if (cf && two) hipLaunchKernelGGL((rtus_tfm_analytic_hmc_kernel<true, true>), grid, block, 0, s, a);
    else if (cf) hipLaunchKernelGGL((rtus_tfm_analytic_hmc_kernel<true, false>), grid, block, 0, s, a);
    else if (two) hipLaunchKernelGGL((rtus_tfm_analytic_hmc_kernel<false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((rtus_tfm_analytic_hmc_kernel<false, false>), grid, block, 0, s, a);
    return hipGetLastError();
}

DasIq rtus_das_iq(double f_demod, double fs);                          // rtus_tfm.hip

hipError_t rtus_launch_tfm_iq_hmc(const float* an, int n_e, int n_t, double fs, double t0, double f_demod, const double* tt_tx,
                                  const double* tt_rx, int n_f, float* image, float* cf, hipStream_t s)
{
    const HmcArgs a = hmc_args(an, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f, image, cf);
    const DasIq iq = rtus_das_iq(f_demod, fs);
    const dim3 grid((n_f + RTUS_BLOCK - 1) / RTUS_BLOCK), block(RTUS_BLOCK);
    const bool two = tt_tx != tt_rx;
    if (cf && two) hipLaunchKernelGGL((rtus_tfm_hmc_iq_kernel<true, true>), grid, block, 0, s, a, iq);
    else if (cf) hipLaunchKernelGGL((rtus_tfm_hmc_iq_kernel<true, false>), grid, block, 0, s, a, iq);
    else if (two) hipLaunchKernelGGL((rtus_tfm_hmc_iq_kernel<false, true>), grid, block, 0, s, a, iq);
    else hipLaunchKernelGGL((rtus_tfm_hmc_iq_kernel<false, false>), grid, block, 0, s, a, iq);
    return hipGetLastError();
}

long long rtus_tfm_frames_blocks(int n_slow, int n_f);                // rtus_tfm_frames.hip

// P frames per block (2: float32 pairs, 4: int16 quads), the blocks cut into launches by rtus_tfm_frames.hip's rule: about 2304
// workgroups per launch, one block per launch from 1153 workgroups per image on.  packed: [n_slow][n_pairs][n_t][P], in 8-byte
// sample positions either way.  No bit depends on the cut: a lane's sums depend on its focal point and its plane only.
#define RTUS_HMCF_LAUNCH_BLOCKS 2304
template <int P>
static hipError_t hmc_frames_launch(const float* packed, int n_frames, int n_e, int n_t, double fs, double t0, const double* tt_tx,
                                    const double* tt_rx, int n_f, float* images, hipStream_t s)
{
    const int n_blk = (int)rtus_tfm_frames_blocks(1, n_f), n_slow = (n_frames + P - 1) / P;
    int m = RTUS_HMCF_LAUNCH_BLOCKS / n_blk > 1 ? RTUS_HMCF_LAUNCH_BLOCKS / n_blk : 1;
    m = m < n_slow ? m : n_slow;
    const size_t block_len = (size_t)n_e * ((size_t)n_e + 1) / 2 * (size_t)n_t * 2;   // floats per block
    for (int q0 = 0; q0 < n_slow; q0 += m) {                          // blocks [q0, q0 + m): frames P q0 .. of the stack
        const int frames = n_frames - P * q0 < P * m ? n_frames - P * q0 : P * m;
        const HmcArgs a = hmc_args(packed + (size_t)q0 * block_len, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f, images + (size_t)(P * q0) * n_f, nullptr);
        const HmcFrames<P> where = {frames, n_blk};
        const dim3 grid((unsigned)rtus_tfm_frames_blocks((frames + P - 1) / P, n_f)), block(RTUS_BLOCK);
        if constexpr (P == 4) {
            if (tt_tx == tt_rx) hipLaunchKernelGGL(rtus_tfm_frames_hmc_i16_kernel<false>, grid, block, 0, s, a, where);
            else hipLaunchKernelGGL(rtus_tfm_frames_hmc_i16_kernel<true>, grid, block, 0, s, a, where);
        } else {
            if (tt_tx == tt_rx) hipLaunchKernelGGL(rtus_tfm_frames_hmc_f32_kernel<false>, grid, block, 0, s, a, where);
            else hipLaunchKernelGGL(rtus_tfm_frames_hmc_f32_kernel<true>, grid, block, 0, s, a, where);
        }
    }
    return hipGetLastError();
}

hipError_t rtus_launch_tfm_frames_hmc_i16(const short* packed, int n_frames, int n_e, int n_t, double fs, double t0, const double* tt_tx,
                                          const double* tt_rx, int n_f, float* images, hipStream_t s)
{
    return hmc_frames_launch<4>((const float*)packed, n_frames, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f, images, s);
}

hipError_t rtus_launch_tfm_frames_hmc(const float* packed, int n_frames, int n_e, int n_t, double fs, double t0, const double* tt_tx,
                                      const double* tt_rx, int n_f, float* images, hipStream_t s)
{
    return hmc_frames_launch<2>(packed, n_frames, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f, images, s);
}

// an output that is not asked for is not computed: vcf null -> no phasor, scf and counts null -> no sign sum
template <bool TWO>
static void hmc_phase_launch(const HmcArgs& a, float* vcf, float* scf, int2* counts, dim3 grid, dim3 block, hipStream_t s)
{
    const bool sign = scf || counts;
    if (vcf && sign) hipLaunchKernelGGL((rtus_tfm_hmc_phase_kernel<true, true, TWO>), grid, block, 0, s, a, HmcPhase<true, true>{vcf, scf, counts});
    else if (vcf) hipLaunchKernelGGL((rtus_tfm_hmc_phase_kernel<true, false, TWO>), grid, block, 0, s, a, HmcPhase<true, false>{vcf, scf, counts});
    else if (sign) hipLaunchKernelGGL((rtus_tfm_hmc_phase_kernel<false, true, TWO>), grid, block, 0, s, a, HmcPhase<false, true>{vcf, scf, counts});
    else hipLaunchKernelGGL((rtus_tfm_hmc_phase_kernel<false, false, TWO>), grid, block, 0, s, a, HmcPhase<false, false>{vcf, scf, counts});
}

hipError_t rtus_launch_tfm_phase_hmc(const float* an, int n_e, int n_t, double fs, double t0, const double* tt_tx, const double* tt_rx,
                                     int n_f, float* image, float* vcf, float* scf, int* counts, hipStream_t s)
{
    const HmcArgs a = hmc_args(an, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f, image, nullptr);
    const dim3 grid((n_f + RTUS_BLOCK - 1) / RTUS_BLOCK), block(RTUS_BLOCK);
    if (tt_tx == tt_rx) hmc_phase_launch<false>(a, vcf, scf, (int2*)counts, grid, block, s);
    else hmc_phase_launch<true>(a, vcf, scf, (int2*)counts, grid, block, s);
    return hipGetLastError();
}

hipError_t rtus_launch_tfm_weighted_hmc(const float* an, int n_e, int n_t, double fs, double t0, const double* tt_tx, const double* tt_rx,
                                        const float* w_tx, const float* w_rx, int n_f, float* image, float* sens, hipStream_t s)
{
    const HmcwArgs g = {hmc_args(an, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f, image, nullptr), (const float2*)w_tx, (const float2*)w_rx, sens};
    const dim3 grid((n_f + RTUS_BLOCK - 1) / RTUS_BLOCK), block(RTUS_BLOCK);
    const bool two = tt_tx != tt_rx;
    if (sens && two) hipLaunchKernelGGL((rtus_tfm_hmc_weighted_kernel<true, true>), grid, block, 0, s, g);
    else if (sens) hipLaunchKernelGGL((rtus_tfm_hmc_weighted_kernel<true, false>), grid, block, 0, s, g);
    else if (two) hipLaunchKernelGGL((rtus_tfm_hmc_weighted_kernel<false, true>), grid, block, 0, s, g);
    else hipLaunchKernelGGL((rtus_tfm_hmc_weighted_kernel<false, false>), grid, block, 0, s, g);
    return hipGetLastError();
}
