// rtus_geomfit.hip — the misfit between rtus_solve's pulse-echo times for a batch of pipe geometries and measured echo times: the
// reference's database search (main_compare.py:526-553: the mean squared error of the hit rays) on any batch of geometries,
// with weights and with the sums a common time offset needs.  Definition in include/rtus.h (rtus_geom_misfit); checked against
// tests/geomfit_numpy.py.
//
// One workgroup = one geometry.  The order of the sums is part of the definition (a geometry's bits must not depend on the batch):
// lane r sums row r (one transmit element) over the receive elements in ascending order, then lane 0 adds the row sums in
// ascending order.  Rows beyond RTUS_BLOCK are taken in further passes of RTUS_BLOCK rows, each pass added after the one before.
// A lane walks its own row, so a wave's 64 loads of one step touch 64 cache lines — and the next fifteen steps hit the same lines:
// the table is read from HBM once (it is small beside the solve that made it: DESIGN §4).
#include "rtus_device.h"

struct MisfitArgs {
    const double* __restrict__ tt;       // [G][T][E]
    const double* __restrict__ tm;       // [T][E]
    const double* __restrict__ w;        // [T][E] or null
    int* __restrict__ n;                 // [G]
    double* __restrict__ sse;            // [G]
    double* __restrict__ sum_r;          // [G]
    double* __restrict__ sum_w;          // [G] or null
    int T, E;
};

__global__ __launch_bounds__(RTUS_BLOCK) void rtus_geom_misfit_kernel(MisfitArgs a)
{
    __shared__ double row_q[RTUS_BLOCK], row_r[RTUS_BLOCK], row_w[RTUS_BLOCK];
    __shared__ int row_n[RTUS_BLOCK];
    const int t = threadIdx.x;
    const double* tt = a.tt + (size_t)blockIdx.x * a.T * a.E;
    double q = 0.0, r = 0.0, sw = 0.0;                       // lane 0's totals
    int n = 0;
    for (int r0 = 0; r0 < a.T; r0 += RTUS_BLOCK) {
        const int row = r0 + t;
        double rq = 0.0, rr = 0.0, rw = 0.0;
        int rn = 0;
        if (row < a.T) {
            const double* x = tt + (size_t)row * a.E;
            const double* m = a.tm + (size_t)row * a.E;
            const double* w = a.w ? a.w + (size_t)row * a.E : nullptr;
            for (int e = 0; e < a.E; ++e) {
                const double wt = w ? w[e] : 1.0;
                const double d = x[e] - m[e];
                if (wt > 0.0 && fabs(d) <= 1.7976931348623157e308) {   // both times finite
#pragma clang fp contract(off)                               // w r is rounded on its own: sum_r adds it, sse multiplies it on
                    const double wd = wt * d;
                    rq = fma(wd, d, rq);
                    rr += wd;
                    rw += wt;
                    ++rn;
                }
            }
        }
        __syncthreads();                                     // the previous pass has been added
        row_q[t] = rq; row_r[t] = rr; row_w[t] = rw; row_n[t] = rn;
        __syncthreads();
        if (t == 0) {
            const int nr = min(RTUS_BLOCK, a.T - r0);
            for (int k = 0; k < nr; ++k) { q += row_q[k]; r += row_r[k]; sw += row_w[k]; n += row_n[k]; }
        }
    }
    if (t == 0) {
        a.n[blockIdx.x] = n;
        a.sse[blockIdx.x] = q;
        a.sum_r[blockIdx.x] = r;
        if (a.sum_w) a.sum_w[blockIdx.x] = sw;
    }
}

hipError_t rtus_launch_geom_misfit(const double* tt, int n_geom, int n_tx, int n_rx, const double* t_meas, const double* w, int* n,
                                   double* sse, double* sum_r, double* sum_w, hipStream_t s)
{
    MisfitArgs a;
    a.tt = tt; a.tm = t_meas; a.w = w; a.n = n; a.sse = sse; a.sum_r = sum_r; a.sum_w = sum_w; a.T = n_tx; a.E = n_rx;
    hipLaunchKernelGGL(rtus_geom_misfit_kernel, dim3(n_geom), dim3(RTUS_BLOCK), 0, s, a);
    return hipGetLastError();
}
