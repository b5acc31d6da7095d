// rtus_skip_reflector.hip — skip legs off a sampled backwall: for every (element e, focal point f) the stationary value over the
// reflector's points j of S_j = tt_down[e, j] + |F_f - B_j| / c_up, refined by a parabola through the three sums about the first
// least one.  rtus_specular's reduction with focal points in the place of receivers and a closed-form up leg in the place of the
// second table: the n_f x n_p table of up legs is never stored.  Definition in include/rtus.h (rtus_skip_reflector); checked bit
// for bit against tests/skip_reflector_numpy.py and against rtus_specular fed with that table.
//
// One workgroup = SKIP_TE elements x 64 focal points.  Lanes own focal points (a wave's stores to a row of tt are 512 consecutive
// bytes); a wave owns SKIP_TE / 4 elements.  The up leg u_j does not depend on the element: per tile of SKIP_JC points each of the
// four waves forms a quarter of u[point][lane] (the reflector's point is wave-uniform: scalar loads, scalar operands) into LDS,
// lane-major, so that writes and reads are 512 consecutive bytes per wave, and all four read it back — u is formed once per
// (focal point, reflector point) and workgroup, not once per element.  The element's row of tt_down is wave-uniform: scalar loads,
// scalar operands in the addition.  A lane carries per element the state of rtus_specular.h; the three sums about j* are formed
// again at the end by the same operations — the same bits.  An entry's bits depend on its own row of tt_down, the reflector and
// its own focal point only: not on the tile it falls into, nor on the launch shape, nor on which outputs are asked for.
#include "rtus_specular.h"

#define SKIP_TE 8                    // elements per workgroup (2 per wave)
#define SKIP_JC 32                   // points per LDS tile (16 KB)
#define SKIP_ROWS (SKIP_TE / (RTUS_BLOCK / RTUS_WAVE))
#define SKIP_FILL (SKIP_JC / (RTUS_BLOCK / RTUS_WAVE))       // points of a tile that one wave forms

struct SkipArgs {
    const double* __restrict__ td;   // [n_e][n_p]
    const double* __restrict__ xb;   // [n_p]
    const double* __restrict__ zb;
    const double* __restrict__ xf;   // [n_f]
    const double* __restrict__ zf;
    double* __restrict__ t;          // [n_e][n_f]
    double* __restrict__ pos;        // or null
    int* __restrict__ n_min;         // or null
    double c, rc;                    // c_up and 1 / c_up, rounded once on the host
    int n_e, n_f, n_p;
    int kt;                          // tiles of focal points
};

// the up leg's time in the header's order: the squares and their sum rounded on their own, the root and the division correctly
// rounded (np.sqrt(dx*dx + dz*dz) / c_up)
__device__ __forceinline__ double skip_up_time(double xf, double zf, double xb, double zb, double c, double rc)
{
#pragma clang fp contract(off)
    const double dx = xf - xb, dz = zf - zb;
    const double r2 = dx * dx + dz * dz;
    return rtus_div_by(rtus_sqrt(r2), c, rc);
}

template <bool COUNT>
__global__ __launch_bounds__(RTUS_BLOCK) void rtus_skip_reflector_kernel(SkipArgs a)
{
    __shared__ double tile[SKIP_JC * RTUS_WAVE];
    const int lane = threadIdx.x & (RTUS_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / RTUS_WAVE);
    const int k = (int)(blockIdx.x % a.kt) * RTUS_WAVE + lane;
    const int i0 = (int)(blockIdx.x / a.kt) * SKIP_TE;
    const bool live = k < a.n_f;
    const double xf = live ? a.xf[k] : __builtin_nan(""), zf = live ? a.zf[k] : __builtin_nan("");

    SpecRow row[SKIP_ROWS];
#pragma unroll
    for (int r = 0; r < SKIP_ROWS; ++r) spec_row_init(row[r]);

    for (int j0 = 0; j0 < a.n_p; j0 += SKIP_JC) {
        const int nj = min(SKIP_JC, a.n_p - j0);
        __syncthreads();                                     // the tile before this one has been read
        const int c1 = min(nj, (wave + 1) * SKIP_FILL);
        for (int c = wave * SKIP_FILL; c < c1; ++c)          // wave-uniform bounds; points past nj are not read below
            tile[c * RTUS_WAVE + lane] = skip_up_time(xf, zf, a.xb[j0 + c], a.zb[j0 + c], a.c, a.rc);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < SKIP_ROWS; ++r) {
            const int i = i0 + wave * SKIP_ROWS + r;         // wave-uniform
            if (i >= a.n_e) continue;
            const double* __restrict__ ar = a.td + (size_t)i * a.n_p + j0;
            SpecRow w = row[r];
#pragma unroll 4                                             // (8, specular's factor, spills 9 SGPRs here: the arguments hold 8 pointers)
            for (int c = 0; c < nj; ++c) spec_row_step<COUNT>(w, spec_finite_or_nan(ar[c] + tile[c * RTUS_WAVE + lane]), j0 + c);
            row[r] = w;
        }
    }

    if (!live) return;
#pragma unroll
    for (int r = 0; r < SKIP_ROWS; ++r) {
        const int i = i0 + wave * SKIP_ROWS + r;
        if (i >= a.n_e) continue;
        const int js = row[r].jbest;
        double t = __builtin_nan(""), p = __builtin_nan("");
        if (js >= 0) {
            p = (double)js;
            if (js > 0 && js < a.n_p - 1) {
                const double* __restrict__ pa = a.td + (size_t)i * a.n_p + js;
                const double sa = pa[-1] + skip_up_time(xf, zf, a.xb[js - 1], a.zb[js - 1], a.c, a.rc);
                const double sb = pa[0] + skip_up_time(xf, zf, a.xb[js], a.zb[js], a.c, a.rc);
                const double sc = pa[1] + skip_up_time(xf, zf, a.xb[js + 1], a.zb[js + 1], a.c, a.rc);
                spec_refine(sa, sb, sc, js, t, p);
            }
        }
        const size_t o = (size_t)i * a.n_f + k;
        a.t[o] = t;
        if (a.pos) a.pos[o] = p;
        if (COUNT) a.n_min[o] = row[r].n_min;
    }
}

// the launcher's grid is one-dimensional: the number of workgroups must fit it
long long rtus_skip_reflector_blocks(int n_e, int n_f)
{
    return (long long)((n_f + RTUS_WAVE - 1) / RTUS_WAVE) * ((n_e + SKIP_TE - 1) / SKIP_TE);
}

hipError_t rtus_launch_skip_reflector(const double* tt_down, int n_e, const double* xb, const double* zb, int n_p, double c_up,
                                      const double* xf, const double* zf, int n_f, double* tt, double* pos, int* n_min, hipStream_t s)
{
    SkipArgs a;
    a.td = tt_down; a.xb = xb; a.zb = zb; a.xf = xf; a.zf = zf; a.t = tt; a.pos = pos; a.n_min = n_min;
    a.c = c_up; a.rc = 1.0 / c_up;
    a.n_e = n_e; a.n_f = n_f; a.n_p = n_p;
    a.kt = (n_f + RTUS_WAVE - 1) / RTUS_WAVE;
    const dim3 grid((unsigned)rtus_skip_reflector_blocks(n_e, n_f));
    if (n_min) hipLaunchKernelGGL(rtus_skip_reflector_kernel<true>, grid, dim3(RTUS_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(rtus_skip_reflector_kernel<false>, grid, dim3(RTUS_BLOCK), 0, s, a);
    return hipGetLastError();
}
