// rtus_specular.hip — specular echo times of sampled reflectors: for every (reflector g, transmitter i, receiver k) the stationary
// value over the reflector's points j of S_j = tt_a[i, g n_p + j] + tt_b[k, g n_p + j], refined by a parabola through the three sums
// about the first least one.  A min-plus product of two travel-time tables (no MFMA applies).  Definition in include/rtus.h
// (rtus_specular); checked bit for bit against tests/specular_numpy.py.
//
// One workgroup = one reflector, SPEC_TI transmit rows, 64 receivers.  Lanes own receivers; a wave owns SPEC_TI / 4 transmit rows.
// The receivers' table goes through LDS in tiles of 64 receivers x SPEC_JC points, transposed on the way in (rows padded by one
// entry: the 16 lanes of a ds_write_b64 group land on 16 different bank pairs), so that the 64 lanes of a wave read 512 consecutive
// bytes at every point.  The transmit row is wave-uniform: its entries arrive by scalar loads and enter the additions as scalar
// operands.  A lane carries, per transmit row, the least sum so far, its index, the previous sum and whether that one fell below
// its predecessor (for n_min); the three sums about j* are formed again from the tables at the end — the same fp64 addition, the
// same bits.  A pair's bits depend on its own two rows only: not on the tile it falls into, nor on the launch shape.
#include "rtus_specular.h"         // spec_finite_or_nan, SpecRow, spec_row_step, spec_refine: shared with rtus_skip_reflector.hip

#define SPEC_TI 8                    // transmit rows per workgroup (2 per wave)
#define SPEC_JC 32                   // points per LDS tile (16.6 KB: eight workgroups per CU, the VGPR limit)
#define SPEC_LD (RTUS_WAVE + 1)      // padded row of the transposed tile [SPEC_JC][SPEC_LD]
#define SPEC_ROWS (SPEC_TI / (RTUS_BLOCK / RTUS_WAVE))

struct SpecArgs {
    const double* __restrict__ ta;   // [n_a][ld]
    const double* __restrict__ tb;   // [n_b][ld]
    double* __restrict__ t;          // [n_refl][n_a][n_b]
    double* __restrict__ pos;        // or null
    int* __restrict__ n_min;         // or null
    int n_a, n_b, n_p;
    int kt, it;                      // tiles of receivers / of transmit rows
    size_t ld;                       // n_refl * n_p
};

__global__ __launch_bounds__(RTUS_BLOCK) void rtus_specular_kernel(SpecArgs a)
{
    __shared__ double tile[SPEC_JC * SPEC_LD];
    const int lane = threadIdx.x & (RTUS_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / RTUS_WAVE);
    unsigned b = blockIdx.x;
    const int k0 = (int)(b % a.kt) * RTUS_WAVE;  b /= a.kt;
    const int i0 = (int)(b % a.it) * SPEC_TI;
    const size_t col0 = (size_t)(b / a.it) * a.n_p;          // the reflector's first column
    const int k = k0 + lane;

    SpecRow row[SPEC_ROWS];
#pragma unroll
    for (int r = 0; r < SPEC_ROWS; ++r) spec_row_init(row[r]);

    for (int j0 = 0; j0 < a.n_p; j0 += SPEC_JC) {
        const int nj = min(SPEC_JC, a.n_p - j0);
        __syncthreads();                                     // the tile before this one has been read
        // stage: thread (c = point, r = receiver) -> tile[c][r]; a wave's 64 loads are 256 consecutive bytes of each of two receivers' rows
        for (int e = threadIdx.x; e < SPEC_JC * RTUS_WAVE; e += RTUS_BLOCK) {
            const int c = e & (SPEC_JC - 1), r = e / SPEC_JC;
            double v = __builtin_nan("");
            if (c < nj && k0 + r < a.n_b) v = a.tb[(size_t)(k0 + r) * a.ld + col0 + j0 + c];
            tile[c * SPEC_LD + r] = v;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < SPEC_ROWS; ++r) {
            const int i = i0 + wave * SPEC_ROWS + r;         // wave-uniform
            if (i >= a.n_a) continue;
            const double* __restrict__ ar = a.ta + (size_t)i * a.ld + col0 + j0;
            SpecRow w = row[r];
#pragma unroll 8
            for (int c = 0; c < nj; ++c) spec_row_step<true>(w, spec_finite_or_nan(ar[c] + tile[c * SPEC_LD + lane]), j0 + c);
            row[r] = w;
        }
    }

    if (k >= a.n_b) return;
    const size_t g = col0 / a.n_p;
#pragma unroll
    for (int r = 0; r < SPEC_ROWS; ++r) {
        const int i = i0 + wave * SPEC_ROWS + r;
        if (i >= a.n_a) continue;
        const int js = row[r].jbest;
        double t = __builtin_nan(""), p = __builtin_nan("");
        if (js >= 0) {
            p = (double)js;
            if (js > 0 && js < a.n_p - 1) {
                const double* __restrict__ pa = a.ta + (size_t)i * a.ld + col0 + js;
                const double* __restrict__ pb = a.tb + (size_t)k * a.ld + col0 + js;
                const double sa = pa[-1] + pb[-1], sb = pa[0] + pb[0], sc = pa[1] + pb[1];
                spec_refine(sa, sb, sc, js, t, p);
            }
        }
        const size_t o = (g * a.n_a + i) * a.n_b + k;
        a.t[o] = t;
        if (a.pos) a.pos[o] = p;
        if (a.n_min) a.n_min[o] = row[r].n_min;
    }
}

hipError_t rtus_launch_specular(const double* tt_a, int n_a, const double* tt_b, int n_b, int n_refl, int n_p, double* t, double* pos,
                                int* n_min, hipStream_t s)
{
    SpecArgs a;
    a.ta = tt_a; a.tb = tt_b ? tt_b : tt_a; a.t = t; a.pos = pos; a.n_min = n_min;
    a.n_a = n_a; a.n_b = n_b; a.n_p = n_p;
    a.kt = (n_b + RTUS_WAVE - 1) / RTUS_WAVE;
    a.it = (n_a + SPEC_TI - 1) / SPEC_TI;
    a.ld = (size_t)n_refl * n_p;
    hipLaunchKernelGGL(rtus_specular_kernel, dim3((unsigned)((size_t)a.kt * a.it * n_refl)), dim3(RTUS_BLOCK), 0, s, a);
    return hipGetLastError();
}

// the launcher's grid is one-dimensional: the number of workgroups must fit it
long long rtus_specular_blocks(int n_a, int n_b, int n_refl)
{
    return (long long)((n_b + RTUS_WAVE - 1) / RTUS_WAVE) * ((n_a + SPEC_TI - 1) / SPEC_TI) * n_refl;
}
