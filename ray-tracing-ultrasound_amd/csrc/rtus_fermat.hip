// rtus_fermat.hip — element x focal-point least-time (Fermat) travel times through horizontal
// layers, one (element, focal point) solve per lane.  NOT IN THE REFERENCE (parity unpinned):
// BASELINE configs 2/3/5 ask for planar interfaces the reference does not model.
//
// Formulation.  Snell's invariant p = sin(theta_i)/c_i.  With cm = fastest traversed speed,
// r_i = c_i/cm, k_i = 1 - r_i^2 and q = tan(theta) in the fastest layer, the horizontal reach is
//     X(q) = sum_i h_i r_i q / sqrt(1 + k_i q^2)          (increasing, concave, X(0) = 0)
//     X'(q) = sum_i h_i r_i (1 + k_i q^2)^(-3/2)
// and the travel time  T(q) = sqrt(1 + q^2) * sum_i (h_i / c_i) / sqrt(1 + k_i q^2).
// Newton on X(q) = |xf - xe| started from a LOWER bound of the root climbs monotonically
// (concavity: the tangent overestimates X), so no bracketing / bisection fallback is needed;
// q stays finite even at grazing incidence (unlike p -> 1/cm).  Convergence is tested per wave
// with a ballot so a wave leaves the loop as soon as all 64 lanes are done.
//
// Cost model (measured on gfx950, scripts/ubench_issue*.hip -> profiles/r02_ubench_issue.txt; cycles per
// wave-instruction per SIMD at 8 waves/SIMD): fp32 fma / mul / add / mov with VGPR or inline-constant operands 2.3;
// the same with an SGPR operand 4.2; every fp64 op, v_cvt, v_max/v_min, v_cmp, v_readlane, v_bfi 4.2; v_rsq_f32 /
// v_rcp_f32 8.2; v_pk_fma_f32 4.2 (packed fp32 buys no issue slots on this part); IEEE fp64 sqrt ~85, divide ~60.
// So the Newton iteration runs entirely on the fp32 pipe with per-lane (VGPR) tables: it only has to bring q within
// 3e-4 of the root — Newton needs neither an exact Jacobian nor an exact residual for that — and the fp64 result is
// produced afterwards; no IEEE sqrt/divide anywhere.
//   * a lane stops when the step it would take is |dq| <= 3e-4 q; it does NOT take that step, so the
//     seeds of its last evaluation belong to its q and are refined (one Newton step in fp64, 1.5 d^2) instead
//     of being recomputed;
//   * T at the exact root follows from the Fermat expansion in the residual dXr = X - X(q):
//     T = T(q) + p dXr + (1/2)(dp/dX) dXr^2,  p = dT/dX = sin(theta)/c  — error O(dXr^3): measured max 3.4e-18 s
//     (median 3e-20 s) against the long-double oracle on BASELINE config 3.
//
// Row table (tau-p tier).  Through horizontal layers T depends on a pair only through the two depths and X = |xf - xe|: a workgroup
// whose 256 targets share one depth (a line of an image grid) and whose elements share another (a linear array) samples ONE
// function T(X).  Such a workgroup, if its block has 32 rows or more, builds a quintic Hermite table of T on the lattice X_j = j h
// (h a power of two chosen from zf - ze alone) from fp64 nodes (T, p, p'), checks every interval against a solved point at
// s = 0.3 to 1e-11 relative, and serves its rows from LDS: ~10 VALU instructions and 48 B of LDS per solve instead of 62 and a
// root-find.  Anything else — mixed depths, a non-finite x, a span beyond 351 intervals, an interval that fails — runs the solver
// exactly as before, the whole workgroup.  A served solve's bits are a function of (X, depths, medium) alone: see "row table: the
// phases".
//
// Structure.  solve_elem is one (element, target) solve; rowtab_point one fp64 node of the table; elem_record one element's record.
// The kernel, rtus_tt_layers_kernel, is a sequence of inlined phases, one function each: work_item (decode), rowtab_ranges or
// solver_records (before the only barrier), rowtab_lattice, rowtab_build, rowtab_serve (the table path), and — where the table is
// not tried or does not serve — solver_records behind a second barrier and solve_block (the element loop).  RowDest says where a
// row of the block is stored, for the serving loop and the solver alike.
//
// Layout: tt[e][f], f fastest — each wave stores 512 contiguous bytes; xf/zf loads are coalesced; the
// per-element data of a workgroup (coordinates, extrapolation weights) sits in LDS and is broadcast to the lanes.
#include "rtus_device.h"

struct LayerArgs {
    double z_if[RTUS_MAX_LAYERS];      // interface depths (n_if used, +inf beyond)
    double c[RTUS_MAX_LAYERS + 1];     // speeds
    double inv_c[RTUS_MAX_LAYERS + 1]; // 1/c (host-computed, correctly rounded)
    int n_if;
    const double* __restrict__ xe;
    const double* __restrict__ ze;
    const double* __restrict__ xf;
    const double* __restrict__ zf;
    double* __restrict__ tt;
    uint8_t* __restrict__ iters;
    int n_e, n_f;
    int eb;                            // elements per workgroup (<= 64): a function of the WHOLE table's size, see rtus_table_rows_per_block
    const int* __restrict__ row_of;    // PERM kernels: output row of element i (the elements arrive sorted by (ze, xe), see rtus_rank_kernel)
    int row0;                          // index of xe[0] in the whole table when this launch solves a block of its rows (else 0):
                                       // workgroups cover rows [k eb, (k + 1) eb) of the WHOLE table, so a row is solved with the
                                       // same predecessors — and comes out with the same bits — whether the table is solved in one
                                       // launch or in row shards
    // batched entry (rtus_tt_layers_batch): problem b = blockIdx.z uses elements / targets / output shifted by these
    long long e_stride, f_stride, t_stride;   // in elements of the respective arrays (0: shared by all problems)
    int gy;                            // blocks of rows in this launch (a launch with the row table flattens columns x row blocks into grid.x)
    long long n_rows;                  // rows of the WHOLE table (a shard's launch: more than its n_e) — the row table's threshold, see work_item
    int rowtab;                        // the launch carries the row table's LDS: tau-p tier and eb >= RTUS_ROWTAB_MIN_ROWS (else no block qualifies)
};

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// Refine an fp32-pipe seed y ~ a^(-1/2) (relative error d <= ~1.5e-7: v_rsq_f32 plus the rounding of its argument)
// with one Newton step in fp64: e = 1 - a y^2,  y <- y (1 + e/2)  -> error 1.5 d^2 <= 4e-14.  On the travel time
// that is < 2e-18 s — an order below the O(dX^3) remainder of the expansion it feeds.
__device__ __forceinline__ double rsqrt_refine(double a, double y)
{
    const double e = fma(-a * y, y, 1.0);
    return fma(y * e, 0.5, y);
}

#ifdef RTUS_EXP_COUNT
static __device__ unsigned long long planar_dbg[8];
extern "C" int rtus_dbg_read_planar(unsigned long long* out)
{
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(out, HIP_SYMBOL(planar_dbg), sizeof(unsigned long long) * 8);
    unsigned long long z[8] = {0};
    hipMemcpyToSymbol(HIP_SYMBOL(planar_dbg), z, sizeof(z));
    return 0;
}
#endif

#ifdef RTUS_EXP_STAMPS   // experiment builds only (scripts/stamps_planar.py): where a row-table workgroup's time goes, phase by phase
#define RTUS_STAMP_WGS 8192
// six stamps per workgroup (rows of eight words): entry, after the records' barrier, after the node pass, after the check pass, first store, last store
static __device__ unsigned long long planar_stamps[RTUS_STAMP_WGS * 8];
extern "C" int rtus_dbg_read_stamps(unsigned long long* out, int n_wg)
{
    if (n_wg < 0 || n_wg > RTUS_STAMP_WGS) return 1;
    void* dev = nullptr;
    const size_t bytes = sizeof(unsigned long long) * 8 * (size_t)n_wg;
    if (hipDeviceSynchronize() != hipSuccess || hipGetSymbolAddress(&dev, HIP_SYMBOL(planar_stamps)) != hipSuccess ||
        hipMemcpy(out, dev, bytes, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    // (cleared for the next launch: a workgroup that took the solver leaves zeros)
    return hipMemset(dev, 0, bytes) == hipSuccess && hipDeviceSynchronize() == hipSuccess ? 0 : 2;
}
// The device's constant-rate clock (100 MHz: the same on every CU), lane 0 of the workgroup, an ordinary vector store.  The row is
// blockIdx.x alone: a batched launch (grid.z > 1) writes every problem's stamps over problem 0's — stamp single-problem launches.
#define RTUS_STAMP(i) do { if (threadIdx.x == 0 && blockIdx.x < RTUS_STAMP_WGS) planar_stamps[blockIdx.x * 8 + (i)] = wall_clock64(); } while (0)
#else
#define RTUS_STAMP(i) do { } while (0)
#endif

// One element's record in LDS: every lane of the workgroup reads the same address (broadcast, no VALU slot —
// a v_readlane costs 4.2 cycles and leaves its value in an SGPR, which halves the rate of every fp32 op reading it).
struct __attribute__((aligned(16))) ElemRec {
    float w1, w2, w3, w4;   // extrapolation weights on the signed solutions of the four previous elements
    double xe;
    int info;               // bits 0-2: previous elements usable as history (0..4); bit 3: depth differs from the previous
                            // element's (layer set-up needed); bit 4: uniform pitch from four elements behind to three ahead (HOLD);
                            // bits 8..: length of the run of 4-history elements starting here
    int row;                // PERM: the element's output row
};

typedef const __attribute__((address_space(3))) ElemRec* RecPtr;   // a record where it lives: LDS (ds_read at a register + immediate offset)

// Relative size of the Newton step at which a lane stops (and does not take it).  A HELD solve of the tau-p tier (HOLD = 2) forms its
// second-order term from quantities good to ~0.1 % (8.4 % at worst): its error is that fraction of (tau^2 / 8) T, so it stops at a third.
#define RTUS_PLANAR_TAU 3e-4f

// Per-lane solver state: the layer table of this lane's target, PERMUTED so that slot 0 is the lane's fastest
// traversed layer (there k = 0 and w = (1 + k q^2)^(-1/2) = 1 exactly: slot 0 needs no rsqrt anywhere).
template <int NL>
struct Lane {
    double hr0, hc0, hr[NL], kk[NL], hc[NL], inv_cm;       // slots 1 .. NL-1 of the arrays are used
    float hr0f, hrf[NL], kkf[NL], rs0f, rhmf, asymf;       // fp32 copies for the Newton loop, cold-start bounds
    float hic;                                             // 1 / (2 cm) (tau-p tail: scales its second-order term)
    float G, dG;                                           // tau-p tail: u^3 / (2 cm X'(q)) of the latest solve + its change per element (see HOLD)
    float tau;                                             // relative step below which a lane stops (+inf: target not below the element)
    float rS3;                                             // 1 / X'(q) of the latest evaluation
};

template <int NL>
__device__ __forceinline__ void layer_setup(const LayerArgs& a, double ze, const double* __restrict__ zf_p, unsigned f8, Lane<NL>& L)
{
    // The target's depth is needed here and nowhere else, and the set-up runs once per depth of the aperture: it is LOADED here (an
    // L2 hit), through an index the compiler cannot see through.  Left to itself it keeps zf — and the parts of the set-up that
    // depend on the target alone, hoisted out of the element loop: four more doubles — in SCRATCH across the loop (no register is
    // free for them): 6 % more HBM writes per launch than the table itself (rocprofv3 WRITE_SIZE), now none.
    asm volatile("" : "+v"(f8));
    const double zf = *(const double*)((const char*)zf_p + f8);   // (the byte offset the stores use anyway: no second index register)
    const bool valid = zf > ze;
    L.tau = valid ? RTUS_PLANAR_TAU : INFINITY;
    // thickness of each layer along the path (0 for layers the path does not enter); fastest speed
    double cm = 0.0, h[NL], hr_l[NL], hc_l[NL], kk_l[NL];   // _l: in layer order
    L.inv_cm = 0.0;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        // (selects, not fmax / fmin: those quiet their operands first — a v_max_f64 of each interface depth with itself, loop-invariant,
        // hoisted and then parked in scratch like zf above; the interface depths are finite or +inf, never NaN)
        const double top = (i == 0) ? ze : (a.z_if[i - 1] > ze ? a.z_if[i - 1] : ze);
        const double bot = (i < NL - 1) ? (a.z_if[i] < zf ? a.z_if[i] : zf) : zf;
        h[i] = fmax(bot - top, 0.0);
        const bool faster = h[i] > 0.0 && a.c[i] > cm;
        cm = faster ? a.c[i] : cm;
        L.inv_cm = faster ? a.inv_c[i] : L.inv_cm;
    }
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const bool fastest = a.c[i] == cm;          // exact: cm IS one of the c[i]
        const double r = fastest ? 1.0 : a.c[i] * L.inv_cm;
        hr_l[i] = h[i] * r;
        hc_l[i] = h[i] * a.inv_c[i];
        kk_l[i] = fastest ? 0.0 : fmax(fma(-r, r, 1.0), 0.0);
    }
    // slot 0 <-> the first layer whose speed is cm (per lane: which layers a path crosses depends on zf)
    int jf = 0;
#pragma unroll
    for (int i = NL - 1; i >= 1; --i) jf = (a.c[i] == cm) ? i : jf;
    jf = (a.c[0] == cm) ? 0 : jf;
    L.hr0 = hr_l[0]; L.hc0 = hc_l[0];
#pragma unroll
    for (int i = 1; i < NL; ++i) {
        const bool sw = i == jf;
        L.hr0 = sw ? hr_l[i] : L.hr0;        L.hc0 = sw ? hc_l[i] : L.hc0;
        L.hr[i] = sw ? hr_l[0] : hr_l[i];    L.hc[i] = sw ? hc_l[0] : hc_l[i];    L.kk[i] = sw ? kk_l[0] : kk_l[i];
    }
#pragma unroll
    for (int i = 1; i < NL; ++i) { L.hrf[i] = (float)L.hr[i]; L.kkf[i] = (float)L.kk[i]; }
    L.hr0f = (float)L.hr0;
    // the two lower bounds of a cold start, formed on the fp32 pipe (they are only a starting guess):
    // X <= s0 q with s0 = X'(0), and X <= hm q + asym — the fastest layer(s) (k = 0) contribute the linear term
    // h q, every slower layer saturates at h r / sqrt(k).  Shaved so that fp32 rounding keeps them lower bounds.
    float s0f = L.hr0f, hmf = L.hr0f, asf = 0.0f;
#pragma unroll
    for (int i = 1; i < NL; ++i) {
        const bool lin = L.kkf[i] == 0.0f;
        s0f += L.hrf[i];
        hmf += lin ? L.hrf[i] : 0.0f;
        asf += lin ? 0.0f : L.hrf[i] * __builtin_amdgcn_rsqf(L.kkf[i]);
    }
    L.rs0f = __builtin_amdgcn_rcpf(s0f) * (1.0f - 4e-6f);
    L.rhmf = __builtin_amdgcn_rcpf(hmf) * (1.0f - 4e-6f);
    L.asymf = asf * (1.0f + 4e-6f);
    L.hic = 0.5f * (float)L.inv_cm;
    L.G = L.dG = 0.0f;
    L.hc0 = valid ? L.hc0 : NAN;                    // target not below the element: T = NaN falls out of the sums
    L.rS3 = 0.0f;
}

// One (element, target) solve.  h1 .. h4: signed solutions qs = sign(xf - xe) q of the four previous elements
// (h1 the latest); the new one is returned.  FAST: the element has four usable predecessors — the cubic extrapolation
// is within 3e-4 of the root for all but ~1e-4 of the solves, so the lower-bound clamp is only formed when a lane
// of the wave asks for a second Newton evaluation.
// TAUP: the travel time from the tau-p form T = p X + sum (h_i / c_i) cos(theta_i) instead of T(q) + its Fermat expansion — see
// the tail below.
template <int NL, bool ITERS, bool FAST, bool TAUP, int HOLD = 0>
__device__ __forceinline__ float solve_elem(uint8_t* __restrict__ iters, Lane<NL>& L, RecPtr R, int hist, double xf,
                                            float h1, float h2, float h3, float h4, bool live, size_t row, unsigned f8,
                                            __amdgpu_buffer_rsrc_t rs, unsigned soff, bool after_held = false, bool* hold_ok = nullptr)
{
    static_assert(HOLD == 0 || (FAST && TAUP), "HOLD is a mode of the tau-p tier's four-history runs");
    const double dxs = xf - R->xe;
    const double X = fabs(dxs);
    // ---- Newton iteration in fp32 -----------------------------------------------------------
    // The loop only has to bring q within tau of the root (the fp64 expansion below removes the
    // rest to third order), so it runs on the fp32 pipe: half the issue cost of fp64 and native
    // v_rsq_f32 / v_rcp_f32.  X(q) = q S1 is evaluated to ~1e-7 relative: noise two orders below
    // the stopping threshold.  Lanes whose target is not below the element carry garbage
    // through the arithmetic (never a step: tau = +inf) and get NaN at the store.
    // FAST (a four-history run) works on the SIGNED problem X(qs) = xf - xe — X(q) = q S1(q^2) is odd, the predictor's history is
    // signed anyway — so the common path has no |.| to materialise and no sign to put back (a v_and and a v_bfi per solve); the
    // rare second-evaluation branch stays signed too and clamps to the signed lower bound (one v_med3_f32).
    float Xf = FAST ? (float)dxs : (float)X;
    double Xt = FAST ? dxs : X;                             // the reach that pairs with q in the tail (same sign as q)
    float y[NL], dq = 0.0f, dXf = 0.0f;                     // dq: the (small, untaken) Newton step of the last evaluation, dXf its residual
    int it = 0;
    // one evaluation of X(q), X'(q) on the fp32 pipe -> Newton step dq; y[] = the rsqrt seeds of this q
    auto eval = [&](float qq, bool second = false) {
        const float q2 = qq * qq;
        float S1 = L.hr0f, S3 = L.hr0f;                     // slot 0: k = 0, y = 1
        const bool held = HOLD == 2 && !second;             // (compile-time where it matters: `second` is a literal at every call)
#pragma unroll
        for (int i = 1; i < NL; ++i) {
            y[i] = __builtin_amdgcn_rsqf(fmaf(L.kkf[i], q2, 1.0f));
            if (held) S1 = fmaf(L.hrf[i], y[i], S1);
            else {
                const float hw = L.hrf[i] * y[i];
                S1 += hw;
                S3 = fmaf(hw, y[i] * y[i], S3);
            }
        }
        // 1 / X'(q): v_rcp_f32 — or, HOLD = 2, the reciprocal of the group's first element as it is (see solve_block).  (Round 3 took
        // ONE Newton step from the previous element's reciprocal instead, error = the change of X' squared: fine on a fine regular
        // pitch, but on a coarse or random one — X' moving by tens of per cent per element, the predictor missing by ~tau — it put
        // 2.8e-10 relative on a table: scripts/fuzz_layers.py --taup with tables large enough for four-history runs found it.)
        if (!held) L.rS3 = __builtin_amdgcn_rcpf(S3);
        dXf = fmaf(-S1, qq, Xf);
        dq = dXf * L.rS3;
    };
    // two lower bounds of the root: X <= X'(0) q, and X <= hm q + asym (shaved so rounding keeps them lower)
    auto lower_bound = [&]() { return fmaxf(fmaxf(fabsf(Xf) * L.rs0f, (fabsf(Xf) - L.asymf) * L.rhmf), 0.0f); };   // (FAST: Xf is signed)
    // Newton from q, every iterate clamped to lb.  A lane is done when the step it WOULD take is small; it does not
    // take it, so y[] stays the y of its q (and a done lane re-derives the same small dq on later trips: no state needed).
    auto newton = [&](float& q, float lb) {
        for (int trip = 0; trip < 64; ++trip) {             // wave-uniform trip count, ballot exit
            eval(q, true);
            const bool big = fabsf(dq) > L.tau * q;         // tau = +inf on lanes without a path: never a step
            if (!__builtin_amdgcn_ballot_w64(big)) break;
            q = big ? fmaxf(q + dq, lb) : q;
            if (ITERS) it += big ? 1 : 0;
        }
    };
    float q;
    if (FAST) {
        // the cubic extrapolation is nearly always within tau of the root: one evaluation, no clamp, no select
        q = fmaf(R->w1, h1, fmaf(R->w2, h2, fmaf(R->w3, h3, R->w4 * h4)));
        eval(q);
#ifdef RTUS_EXP_COUNT   // experiment builds only (scripts/exp_planar_miss.py): how far the cubic predictor lands from the root
        if (live && L.tau < 1.0f) {
            const float rel = fabsf(dq) / fabsf(q);
            atomicAdd(&planar_dbg[0], 1ull);
            if (rel > 3e-5f) atomicAdd(&planar_dbg[1], 1ull);
            atomicMax((unsigned long long*)&planar_dbg[7], (unsigned long long)__float_as_uint(rel));
        }
        {   // waves with any lane beyond 3e-5 / 5e-5 / 1e-4
            const float relw = (live && L.tau < 1.0f) ? fabsf(dq) / fabsf(q) : 0.0f;
            const bool l0 = (threadIdx.x & 63) == 0;
            if (__ballot(relw > 3e-5f) && l0) atomicAdd(&planar_dbg[2], 1ull);
            if (__ballot(relw > 5e-5f) && l0) atomicAdd(&planar_dbg[3], 1ull);
            if (__ballot(relw > 1e-4f) && l0) atomicAdd(&planar_dbg[4], 1ull);
        }
#endif
        // (a prediction of the wrong sign is never "small": the step it asks for is larger than itself).  A held solve stops at tau / 3
        // on the second-evaluation path too: its error bound is one at the stopping threshold, whatever the predictor left it.
        const float tau_f = HOLD == 2 ? L.tau * (1.0f / 3.0f) : L.tau;   // (loop-invariant: one register, no instruction per solve)
        const bool big = fabsf(dq) > tau_f * fabsf(q);
        if (__builtin_amdgcn_ballot_w64(big)) {             // wave-uniform: some lane wants a second evaluation
            asm volatile("" : "+v"(q));                     // keeps this block a branch (nothing of it is speculated)
            // Newton on the signed problem, clamped to the signed lower bound: max(., lb) for targets to the right of the element,
            // min(., -lb) to the left = the median with that side's infinity (one v_med3_f32 either way)
            const float sgb = __int_as_float(__double2hiint(dxs));
            const float lbs = __builtin_copysignf(lower_bound(), sgb), sinf = __builtin_copysignf(INFINITY, sgb);
            q = big ? __builtin_amdgcn_fmed3f(q + dq, lbs, sinf) : q;
            if (ITERS) it += big ? 1 : 0;
            for (int trip = 0; trip < 64; ++trip) {         // wave-uniform trip count, ballot exit
                eval(q, true);
                const bool bigger = fabsf(dq) > tau_f * fabsf(q);
                if (!__builtin_amdgcn_ballot_w64(bigger)) break;
                q = bigger ? __builtin_amdgcn_fmed3f(q + dq, lbs, sinf) : q;
                if (ITERS) it += bigger ? 1 : 0;
            }
        }
    } else {
        const float lb = lower_bound();
        q = lb;
        if (hist > 0)                                       // wave-uniform; unused weights are 0
            q = fmaxf(fabsf(fmaf(R->w1, h1, fmaf(R->w2, h2, fmaf(R->w3, h3, R->w4 * h4)))), lb);
        newton(q, lb);
    }
    // ---- fp64: accurate T at q + the Fermat expansion in the residual dXr = X - X(q) ----------
    // T(root) = T(q) + p dXr + (1/2) (dp/dX) dXr^2 + O(dXr^3),
    // p = sin(theta)/cm = q u / cm,  dp/dX = u^3 / (cm X'(q)),  u = 1/sqrt(1+q^2).
    const double qd = (double)q;
    const double q2 = qd * qd;
    const double a1 = 1.0 + q2;
    const float us = __builtin_amdgcn_rsqf(fmaf(q, q, 1.0f));   // u to 1e-7 on the fp32 pipe: seed + 2nd-order term
    const double u = rsqrt_refine(a1, (double)us);
    double T;
    if (!TAUP) {
        double A1 = L.hr0, ST = L.hc0;                      // slot 0: w = 1
#pragma unroll
        for (int i = 1; i < NL; ++i) {
            const double w = rsqrt_refine(fma(L.kk[i], q2, 1.0), (double)y[i]);
            A1 = fma(L.hr[i], w, A1);
            ST = fma(L.hc[i], w, ST);
        }
        const double dXr = fma(-A1, qd, Xt);
        // T = T(q) + dXr (u/cm) (q + (u^2 / (2 X'(q))) dXr) = u (a1 ST + (dXr / cm) (q + s2 dXr)): the coefficient s2 only
        // scales the 2nd-order term (relative size (dXr/X)^2 ~ 1e-7), so it is formed on the fp32 pipe from the seeds.
        const float s2 = (0.5f * us) * (us * L.rS3);
        T = u * fma(L.inv_cm, dXr * fma((double)s2, dXr, qd), a1 * ST);
    } else {
        // tau-p form (the faster accuracy tier, RTUS_TT_TAUP_TAIL): with p = sin(theta)/c = q u / cm and cos(theta_i) =
        // u sqrt(1 + k_i q^2), F(p) = p X + sum (h_i/c_i) cos(theta_i) is STATIONARY in p at the ray (dF/dp = X - X(p)): evaluated
        // at the Newton iterate its first-order error vanishes by itself — no second weighted sum (X(q) in fp64), no fp64
        // residual — and T = F + (1/2)(dp/dX) dXr^2 with the residual the fp32 evaluation already has:
        // (1/2)(dp/dX) dXr^2 = (1/2) u^3 / (cm X') dXr^2 = (1/2) u^3 (dq dXr) / cm.  The fp32 residual carries ~2e-7 X of
        // rounding, so that term — and T — is off by up to (dq/q) 2e-7 T: 6e-11 T at the stopping threshold, ~3e-14 T typically
        // (the accurate tier: 1e-13 T at most).  Four fp64 instructions fewer per solve (24 against 28 with three layers).
        double ST = L.hc0;                                  // slot 0: cos(theta_0) / u = 1
#pragma unroll
        for (int i = 1; i < NL; ++i) {
            const double d = fma(L.kk[i], q2, 1.0), yi = (double)y[i];
            const double g = d * yi;                        // sqrt(d) from the seed ...
            const double t = fma(-g, g, d) * yi;            // ... and one Newton step: sqrt(d) = g + t / 2 (error ~1e-14)
            ST = fma(L.hc[i], fma(t, 0.5, g), ST);
        }
        // the second-order term = G dXf^2 with G = u^3 / (2 cm X'(q)); HOLD = 2: the G of the group's first element (see solve_block)
        float G;
        if (HOLD == 2) G = L.G = L.G + L.dG;                // one element further along the secant through the last two G formed exactly
        else {
            G = ((L.hic * us) * (us * us)) * L.rS3;
            if (HOLD == 1) {
                // the secant through the two latest EXACTLY formed G.  After a held group L.G is the extrapolated G of the element
                // before this one, and L.G - 3 dG the exact G of the previous group's first element, four elements back; otherwise
                // L.G is the exact G of the element before this one.  (after_held is wave-uniform: two scalar selects, one FMA.)
                L.dG = fmaf(after_held ? 3.0f : 0.0f, L.dG, G - L.G) * (after_held ? 0.25f : 1.0f);
                // G is a smooth function of q (|d ln G / dq| <= 3, |G'' / G| <= ~20 along the aperture).  With the root moving by
                // Dq <= 0.02 per element, the secant through the G of elements -s and 0 misses the G of element j by at most
                // |G''| (j + s) j Dq^2 / 2: over the three elements ahead (j <= 3) 10.5 |G''| Dq^2 <= 8.4 % of G after a held group
                // (s = 4), 6 |G''| Dq^2 <= 4.8 % after one that was not (s = 1) — typically ~0.1 %.  The test also rules out a
                // group that straddles the extremum of G under a target (first difference ~0, second difference not).  (A separate
                // test on the first difference of G was redundant with this one: dropped.)
                *hold_ok = !__builtin_amdgcn_ballot_w64(fabsf(h1 - h2) > 0.02f) &&   // (lanes without a path: NaN, never true)
                           (__builtin_amdgcn_readfirstlane(R->info) & 16);            // the pitch is uniform around this group
            }
            L.G = G;
        }
        const float Sf = (G * dXf) * dXf;
        T = fma(u, fma(qd * L.inv_cm, Xt, ST), (double)Sf);
    }
    // store through the workgroup's buffer descriptor (base: its first output row, extent: its block of rows): the
    // element's row enters as the scalar offset, each lane supplies a 32-bit byte offset (no 64-bit per-lane address
    // arithmetic, no descriptor rebuilt per row); lanes beyond the last target have redone the last target and store
    // to its address (gfx950 range-checks scalar + lane offset together, so a one-row extent cannot drop them)
    {
        const u32x2 bits = {(unsigned)__double2loint(T), (unsigned)__double2hiint(T)};
        __builtin_amdgcn_raw_buffer_store_b64(bits, rs, f8, soff, 0);        // f8: the target's byte offset in a row (8 f)
        if (ITERS && live) (iters + row)[f8 >> 3] = (uint8_t)it;
    }
    // history for the predictor (fp32): the root itself, q + (untaken step), with the sign of xf - xe (FAST: it has it)
    const float qroot = q + dq;
    return FAST ? qroot : __builtin_copysignf(qroot, __int_as_float(__double2hiint(dxs)));    // one v_bfi_b32
}

// ---- Row table (tau-p tier) ------------------------------------------------------------------------------------------------
// Through horizontal layers T depends on an (element, target) pair only through the two depths and X = |xf - xe|.  On an image
// grid the 256 targets of a workgroup share one depth, on a linear array its elements share another: the workgroup's solves are
// samples of ONE smooth function T(X).  Such a workgroup tabulates it — a quintic Hermite interpolant on a lattice, from fp64
// nodes, every interval verified against a solved point — and serves its rows from the table: a subtract, an exact index, 48 B
// from LDS and five FMAs per solve instead of a root-find.  scripts/study_planar_rowtable.py is the CPU emulation that settled
// the divisor, the capacity and the bound; DESIGN.md section 4 "Row table" has the error budget and the measurements.
#define RTUS_ROWTAB_SLOTS 352          // 48-byte intervals per workgroup: 16.5 KB + the records = 19 KB, eight workgroups per CU in 160 KB
#define RTUS_ROWTAB_MIN_ROWS 32        // rows of the block below which the table does not pay: building it costs each lane two fp64 solves,
                                       // the coefficients and the reductions (~800 instructions), a served row saves ~48 of the solver's 62
                                       // -> even at ~17 rows; twice that, so that a block which qualifies wins clearly
#define RTUS_ROWTAB_DIV (1.4142135623730951 / 128.0)   // h = the power of two nearest (in ratio) to (zf - ze) / 128
#define RTUS_ROWTAB_CHECK_S 0.3        // where an interval is checked: OFF centre (at s = 1/2 an error common to both nodes' p cancels)
#define RTUS_ROWTAB_BOUND 1e-11        // relative bound of that check: with the error shape s^3 (1 - s)^3 (0.59 of its maximum at s = 0.3)
                                       // a passing interval is within 1.7e-11 everywhere, + 1e-13 of node error: under the tier's 6e-11
#define RTUS_ROWTAB_RESID 1e-13        // fp64 residual |X - X(q)| / X at which a node's Newton iteration stops

struct __attribute__((aligned(16))) RowTabSlot { double c[6]; };   // T on [X_j, X_j + h] = sum c_k s^k, s = (X - X_j) / h
struct RowTabHdr {
    double flo[4], fhi[4];             // per wave: range of its targets' x
    double elo, ehi, ze;               // range of the block's element x, their depth
    int fok[4];                        // per wave: every target at the workgroup's first target's depth, every xf finite
    int eok;                           // every element at the first one's depth, every xe finite
    int bad[4];                        // per wave: a node that did not converge or an interval that failed its check
};

__device__ __forceinline__ double wave_min_f64(double v) { for (int m = 32; m; m >>= 1) v = fmin(v, __shfl_xor(v, m)); return v; }
__device__ __forceinline__ double wave_max_f64(double v) { for (int m = 32; m; m >>= 1) v = fmax(v, __shfl_xor(v, m)); return v; }

// T, p = dT/dX and p' = dp/dX at reach X, to fp64: the solver's fp32 Newton iteration from the lower bound of the root, then Newton
// steps in fp64 until |X - X(q)| <= 1e-13 X (seeds from the fp32 pipe, refined twice: no IEEE sqrt or divide).  A function of
// (X, L) alone — a lane that is done keeps its q while the wave goes on, so its result does not depend on its neighbours'.
// Returns false when the residual was not reached (the caller gives the table up).
template <int NL>
__device__ __forceinline__ bool rowtab_point(const Lane<NL>& L, double X, double& T, double& p, double& pp)
{
    const float Xf = (float)X;
    const float lb = fmaxf(fmaxf(Xf * L.rs0f, (Xf - L.asymf) * L.rhmf), 0.0f);
    float q = lb;
    for (int trip = 0; trip < 64; ++trip) {                 // wave-uniform trip count, ballot exit
        const float q2 = q * q;
        float S1 = L.hr0f, S3 = L.hr0f;
#pragma unroll
        for (int i = 1; i < NL; ++i) {
            const float y = __builtin_amdgcn_rsqf(fmaf(L.kkf[i], q2, 1.0f));
            const float hw = L.hrf[i] * y;
            S1 += hw;
            S3 = fmaf(hw, y * y, S3);
        }
        const float dq = fmaf(-S1, q, Xf) * __builtin_amdgcn_rcpf(S3);
        const bool big = fabsf(dq) > RTUS_PLANAR_TAU * q;
        if (!__builtin_amdgcn_ballot_w64(big)) break;
        q = big ? fmaxf(q + dq, lb) : q;
    }
    double qd = (double)q, S1 = 0.0, S3 = 0.0, ST = 0.0, q2 = 0.0;   // ST: sum (h_i / c_i) cos(theta_i) / u, formed with the sums (no w[] kept)
    bool ok = false;
    for (int trip = 0; trip < 8; ++trip) {
        q2 = qd * qd;
        S1 = S3 = L.hr0;
        ST = L.hc0;
#pragma unroll
        for (int i = 1; i < NL; ++i) {
            const double d = fma(L.kk[i], q2, 1.0);
            const double w = rsqrt_refine(d, rsqrt_refine(d, (double)__builtin_amdgcn_rsqf((float)d)));
            const double hw = L.hr[i] * w;
            S1 += hw;
            S3 = fma(hw, w * w, S3);
            ST = fma(L.hc[i] * d, w, ST);
        }
        const double dX = fma(-S1, qd, X);
        ok = fabs(dX) <= RTUS_ROWTAB_RESID * X;              // (NaN: never)
        if (!__builtin_amdgcn_ballot_w64(!ok)) break;
        double r = (double)__builtin_amdgcn_rcpf((float)S3);
        r = fma(fma(-S3, r, 1.0), r, r);
        qd = ok ? qd : fma(dX, r, qd);                      // (a lane that is done stays where it is: the sums remain those of its q)
    }
    double r = (double)__builtin_amdgcn_rcpf((float)S3);
    r = fma(fma(-S3, r, 1.0), r, r);
    r = fma(fma(-S3, r, 1.0), r, r);
    const double a1 = 1.0 + q2;
    const double u = rsqrt_refine(a1, rsqrt_refine(a1, (double)__builtin_amdgcn_rsqf((float)a1)));
    p = qd * u * L.inv_cm;
    T = fma(p, X, u * ST);                                  // the tau-p form: stationary in q, the residual enters squared
    pp = (u * u) * (u * L.inv_cm) * r;
    return ok;
}

// The positions a record is formed from: an element and its four predecessors inside the workgroup's block (one element per lane
// of the first wave).  All loads are issued together.
struct ElemPos { double x0, x1, x2, x3, x4, z0, z1, z2, z3, z4; };
__device__ __forceinline__ ElemPos load_elem_pos(const double* __restrict__ xe_p, const double* __restrict__ ze_p, int e0, int el)
{
    const int b1 = max(el - 1, e0), b2 = max(el - 2, e0), b3 = max(el - 3, e0), b4 = max(el - 4, e0);
    ElemPos P;
    P.x0 = xe_p[el]; P.z0 = ze_p[el];
    P.x1 = xe_p[b1]; P.x2 = xe_p[b2]; P.x3 = xe_p[b3]; P.x4 = xe_p[b4];
    P.z1 = ze_p[b1]; P.z2 = ze_p[b2]; P.z3 = ze_p[b3]; P.z4 = ze_p[b4];
    return P;
}

// The solver's record of one element (lane `lane` of the first wave, all 64 lanes active: the ballots below are the wave's): how much
// history it has, the predictor's weights, the length of the four-history run that starts at it, whether HOLD may run over it.
template <bool TAUP>
__device__ __forceinline__ ElemRec elem_record(const LayerArgs& a, int lane, int ne, const ElemPos& P, int row)
{
    const double x0 = P.x0, x1 = P.x1, x2 = P.x2, x3 = P.x3, x4 = P.x4, z0 = P.z0, z1 = P.z1, z2 = P.z2, z3 = P.z3, z4 = P.z4;
    // how many predecessors inside this workgroup share the element's depth (the history restarts when ze changes)
    // (a predecessor at a non-finite position is no history either — its solution is NaN, and 0 x NaN in the predictor's unused
    // terms would carry it into up to four rows behind it: scripts/exp_nan_rows.py, tests/test_gpu_edge_sizes.py)
    const bool s1 = (lane >= 1) & (z1 == z0) & isfinite(x1), s2 = s1 & (lane >= 2) & (z2 == z0) & isfinite(x2),
               s3 = s2 & (lane >= 3) & (z3 == z0) & isfinite(x3), s4 = s3 & (lane >= 4) & (z4 == z0) & isfinite(x4);
    int hist = s4 ? 4 : (s3 ? 3 : (s2 ? 2 : (s1 ? 1 : 0)));
    // Lagrange weights of the extrapolation to x0 from the nodes x1 .. x_m (differences in fp64, products in fp32)
    const float t1 = (float)(x0 - x1), t2 = (float)(x0 - x2), t3 = (float)(x0 - x3), t4 = (float)(x0 - x4);
    const float d12 = (float)(x1 - x2), d13 = (float)(x1 - x3), d14 = (float)(x1 - x4), d23 = (float)(x2 - x3),
                d24 = (float)(x2 - x4), d34 = (float)(x3 - x4);
    // duplicate positions leave no slope: use as many nodes as are pairwise distinct, at least the latest one
    const bool ok2 = d12 != 0.0f, ok3 = ok2 & (d13 != 0.0f) & (d23 != 0.0f),
               ok4 = ok3 & (d14 != 0.0f) & (d24 != 0.0f) & (d34 != 0.0f);
    const int m = (hist >= 4 && ok4) ? 4 : ((hist >= 3 && ok3) ? 3 : ((hist >= 2 && ok2) ? 2 : (hist >= 1 ? 1 : 0)));
    float w1 = 0.0f, w2 = 0.0f, w3 = 0.0f, w4 = 0.0f;
    if (m == 4) {
        w1 = t2 * t3 * t4 / (d12 * d13 * d14);
        w2 = -t1 * t3 * t4 / (d12 * d23 * d24);
        w3 = t1 * t2 * t4 / (d13 * d23 * d34);
        w4 = -t1 * t2 * t3 / (d14 * d24 * d34);
    } else if (m == 3) {
        w1 = t2 * t3 / (d12 * d13);
        w2 = -t1 * t3 / (d12 * d23);
        w3 = t1 * t2 / (d13 * d23);
    } else if (m == 2) {
        w1 = t2 / d12;
        w2 = -t1 / d12;
    } else if (m == 1) {
        w1 = 1.0f;
    }
    // run of consecutive elements (from this one on) that all have four distinct same-depth predecessors
    const unsigned long long m4 = __ballot(m == 4 && lane < ne);
    const unsigned long long rest = ~(m4 >> lane);
    const int run = (m == 4 && lane < ne) ? (rest ? __ffsll((long long)rest) - 1 : 64 - lane) : 0;
    // HOLD (tau-p tier) extrapolates along the ELEMENT INDEX: only where the pitch is uniform (2 %) over the four elements behind
    // and the three ahead (an aperture of random spacing put 4.5e-9 relative on a table before this test existed —
    // tests/test_gpu_irregular_apertures.py::test_planar_taup_tier_irregular_and_coarse_apertures).  Behind: this lane's own
    // differences; ahead: the same statement of the lane three further on (they share the step x_i - x_(i-1)).  No loads, no LDS
    // word of its own: the workgroup's start-up is not overlapped with anything (0.1 us there is 1 % of a configs[1] launch).
    bool uni = false;
    if (TAUP && a.eb >= 8) {                            // (a block of fewer rows has no group of four behind four cold rows)
        const float tolu = 0.02f * fabsf(t1);
        const bool ub = m == 4 && lane < ne && fabsf(d12 - t1) <= tolu && fabsf(d23 - t1) <= tolu && fabsf(d34 - t1) <= tolu;
        const unsigned long long ubm = __ballot(ub);
        uni = __builtin_amdgcn_inverse_ballot_w64(ubm & (ubm >> 3));
    }
    ElemRec r;
#ifdef RTUS_EXP_BAD_PREDICTOR                               // experiment builds only (scripts/selftest_predictor.sh): the continuation tests must notice
    w1 *= 1.02f; w3 *= 0.97f;
#endif
    r.w1 = w1; r.w2 = w2; r.w3 = w3; r.w4 = w4; r.xe = x0;
    r.info = m | (hist == 0 ? 8 : 0) | (uni ? 16 : 0) | (run << 8);
    r.row = row;
    return r;
}

// ---- The kernel's phases ---------------------------------------------------------------------------------------------------
// A workgroup = 256 focal points x `eb` consecutive elements (loop).  Besides re-using the layer
// set-up while ze repeats, the loop gives each lane a CONTINUATION PREDICTOR: the signed solution
// qs = sign(xf - xe) q is a smooth function of the element position, so the four previous
// solutions extrapolate the next one (cubic Lagrange form on the actual element positions) to ~1e-5 .. 1e-7
// and Newton needs one evaluation instead of ~4.5.  The weights depend on the element positions only: thread t of
// the workgroup works them out once for element e0 + t and parks them in LDS.
// The predictor is only a guess: iterates are clamped to the rigorous lower bound of the root,
// from which Newton is monotone, so convergence never depends on the elements being evenly spaced.
// The kernel (at the end of this part) is a sequence of the functions below: decode the work item; before the only barrier leave
// either the solver's records or, where the row table is tried, the ranges it is decided on; choose the lattice, build and verify
// the table and serve the rows from it; failing that, form the records behind a second barrier and run the solver over the block.
// Every function is inlined into the kernel; the LDS they share is the kernel's and is handed down by pointer.

// A work item = (column of 256 targets, block of rows, problem of a batch): one per workgroup, decoded once.
struct WorkItem {
    const double* __restrict__ xe;     // the problem's arrays (a batched launch: problem blockIdx.z)
    const double* __restrict__ ze;
    const double* __restrict__ xf;
    const double* __restrict__ zf;
    double* __restrict__ tt;
    uint8_t* __restrict__ iters;       // (ITERS kernels, else null)
    int bx;                            // the column of targets
    int f;                             // this lane's target; lanes beyond the last target redo the last one (live = false)
    unsigned f8;                       // its byte offset in a row of the table (n_f x 8 < 2^32: the launcher checks)
    bool live;
    int gb;                            // the workgroup's block of the whole table
    int e0, ne;                        // its first element in this launch's rows, and how many (<= 64)
    bool try_tab;                      // the row table is tried
};

template <bool ITERS, bool ROWTAB>
__device__ __forceinline__ WorkItem work_item(const LayerArgs& a)
{
    // A launch that carries the row table hands its work items out ALONG THE ROW BLOCKS first (blockIdx.x = bx gy + by: launch_layers
    // flattens its grid): workgroups that start together then write into gy row blocks at once instead of into neighbouring 2-KB
    // pieces of the same rows, which is what the store stream wants (DESIGN.md section 4 "Store stream").  Other launches keep x first.
    // Within every whole group of four columns the two middle ones change places (bits 0 and 1 of the column swapped): workgroups are
    // dealt round-robin over the eight XCDs, so with gy = 4 (the 64-row regime's 256-row table) XCD k would hold by = k mod 4 and every
    // SECOND 2-KB piece of its rows for the whole launch; with the swap its pieces come in adjacent pairs, 4 KB.  Measured: -4.4 us of
    // 98 (DESIGN.md section 4 "Order across rows and XCDs").  A permutation of the columns inside the window that is in flight: with
    // another gy the XCDs are dealt other columns and no gain was measured.  The ragged last group (gx no multiple of four) keeps its order.
    int bx = a.rowtab ? (int)(blockIdx.x / (unsigned)a.gy) : (int)blockIdx.x;
    if (ROWTAB && a.rowtab && (bx | 3) < (a.n_f + RTUS_BLOCK - 1) / RTUS_BLOCK) bx = (bx & ~3) | ((bx & 1) << 1) | ((bx >> 1) & 1);
    const int by = a.rowtab ? (int)(blockIdx.x % (unsigned)a.gy) : (int)blockIdx.y, bz = blockIdx.z;
    WorkItem wi;
    wi.bx = bx;
    wi.xe = a.xe + (size_t)bz * a.e_stride;
    wi.ze = a.ze + (size_t)bz * a.e_stride;
    wi.xf = a.xf + (size_t)bz * a.f_stride;
    wi.zf = a.zf + (size_t)bz * a.f_stride;
    wi.tt = a.tt + (size_t)bz * a.t_stride;
    wi.iters = ITERS ? a.iters + (size_t)bz * a.t_stride : nullptr;
    const int f_raw = bx * RTUS_BLOCK + threadIdx.x;
    wi.live = f_raw < a.n_f;
    wi.f = wi.live ? f_raw : a.n_f - 1;
    wi.f8 = (unsigned)wi.f * 8u;
    wi.gb = a.row0 / a.eb + by;
    wi.e0 = max(wi.gb * a.eb - a.row0, 0);                   // (a shard that starts inside a block keeps its tail)
    wi.ne = min((wi.gb + 1) * a.eb - a.row0, a.n_e) - wi.e0;
    // Row table: tried where the block OF THE WHOLE TABLE has enough rows for it to pay (a scalar test on the launch's arguments:
    // a table of short blocks, configs[1] for one, pays nothing further).
    wi.try_tab = ROWTAB && a.rowtab && min((long long)(wi.gb + 1) * a.eb, a.n_rows) - (long long)wi.gb * a.eb >= RTUS_ROWTAB_MIN_ROWS;
    return wi;
}

// Where element `idx` of the block is stored: its row inside the workgroup's block of rows (one descriptor, the row as the
// instruction's scalar offset) or, PERM, a descriptor of the row it belongs to (a few scalar instructions per element).  The callers
// walk the block and pass the running offsets of row idx — `off` in elements from the table's start, `soff` in bytes from the block's.
template <bool PERM>
struct RowDest {
    double* __restrict__ tt;
    const ElemRec* rec;                // PERM: the records hold each element's row
    size_t nf, o0;                     // elements per row; offset of the block's first row (wave-uniform)
    unsigned row_bytes;                // (li x row_bytes < 2^32: the launcher sizes eb for it)
    __amdgpu_buffer_rsrc_t rs;         // the block's rows
    __device__ __forceinline__ size_t row(int idx, size_t off) const    // the row's offset: of the iteration counts too
    {
        return PERM ? (size_t)(unsigned)__builtin_amdgcn_readfirstlane(rec[idx].row) * nf : off;
    }
    __device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(int idx, size_t off) const
    {
        if (!PERM) return rs;
        return __builtin_amdgcn_make_buffer_rsrc(tt + row(idx, off), 0, row_bytes, 0x00020000);
    }
    __device__ __forceinline__ unsigned soff(unsigned off) const { return PERM ? 0u : off; }
};

template <bool PERM>
__device__ __forceinline__ RowDest<PERM> row_dest(const LayerArgs& a, const WorkItem& wi, const ElemRec* rec)
{
    RowDest<PERM> d;
    d.tt = wi.tt; d.rec = rec;
    d.nf = (size_t)a.n_f;
    d.o0 = (size_t)wi.e0 * d.nf;
    d.row_bytes = (unsigned)a.n_f * 8u;
    d.rs = __builtin_amdgcn_make_buffer_rsrc(wi.tt + d.o0, 0, (unsigned)wi.ne * d.row_bytes, 0x00020000);
    return d;
}

// The solver's records of the block: the first wave works them out, one element per lane (`el`: the lane's element).  Called before
// the only barrier where the table is not tried (nothing waits on the targets there), and behind a second barrier where it was tried
// and does not serve.
template <bool TAUP, bool PERM>
__device__ __forceinline__ void solver_records(const LayerArgs& a, const WorkItem& wi, int el, ElemRec* rec)
{
    rec[threadIdx.x] = elem_record<TAUP>(a, threadIdx.x, wi.ne, load_elem_pos(wi.xe, wi.ze, wi.e0, el), PERM ? a.row_of[el] : 0);
}

// ---- row table: the phases -------------------------------------------------------------------------------------------------
// ELIGIBLE: every target of the workgroup at one depth zf, every element of the block at one depth ze < zf, every x finite, the
// block long enough (try_tab).  LATTICE: nodes X_j = j h anchored at X = 0, h the power of two nearest (zf - ze) / 128: a
// function of the two depths alone.  The workgroup builds the intervals [tlo, thi] that its |xf - xe| can touch — from the
// extreme pairs: fl(xf - xe) is monotone in both, so every solve's index floor(X / h) lies between theirs and no lane needs a
// range check — one node per lane (T, h p, h^2 p' / 2: the first three coefficients of the interval that starts there), then
// one interval per lane: the upper three coefficients from the two nodes, and a solved point at s = 0.3 against the
// interpolant.  A node that did not reach its residual, an interval beyond 1e-11, more intervals than the table holds: the
// WHOLE workgroup takes the solver path, before a row is stored (its history needs every row).
// BITS.  A served solve is a function of (X, j, h, the depths, the medium): X / h, X / h - tlo and the fraction are exact, a
// node is solved cold from X_j, an interval's coefficients come from its own two nodes — no trace of tlo, of the lane that
// built it, of the launch.  So a row served here has the same bits from one launch, from row shards, from the batched entry
// and from the sorted entry in any order of the aperture, and the row of an element at +x mirrors that of one at -x.  What is
// left is the DECISION, which must not depend on the launch either.  It is a function of the block's rows: of their number
// IN THE WHOLE TABLE (gb, eb, n_rows: not the rows this launch holds), and of conditions that are all MONOTONE in the set of
// elements — one depth, finite x, [tlo, thi] inside the capacity, every interval of [tlo, thi] good (an interval's verdict is
// a function of j).  A launch that holds the whole block (any shard cut at multiples of eb, the batched and the sorted
// entries) decides on the same elements as the whole table's launch.  One that holds PART of a block sees a subset: where the
// whole block qualifies so does every part of it, and the rows agree bit for bit wherever the shard is cut; where the whole
// block does not, the whole table's launch ran the solver — whose bits in a block cut apart were never those of the whole
// (its history starts at the cut: rtus_launch_tt_layers_rows promises equal bits for cuts at multiples of eb only).

// Before the only barrier.  Each wave leaves the range of its targets' x and whether they share the first target's depth; the first
// wave does the same for the elements.  A workgroup that tries the table forms the solver's records only if it turns out to need
// them: here it leaves what serving reads — the element's position and, PERM, its row — and the header's words.  Returns the depth
// of the lane's target.
template <bool PERM>
__device__ __forceinline__ double rowtab_ranges(const LayerArgs& a, const WorkItem& wi, double xf, int el, ElemRec* rec, RowTabHdr& hdr)
{
    const bool first_wave = threadIdx.x < 64;
    // The first wave's element loads go out WITH the targets', before anything waits on either: behind the wait for xf and zf,
    // which the reductions need, they were a second round trip to the L2 with three waves at the barrier meanwhile.
    ElemPos P;                                               // (the first wave's, x0 and z0 alone: no other wave reads it)
    int prow = 0;
    if (first_wave) {
        P.x0 = wi.xe[el]; P.z0 = wi.ze[el];
        if (PERM) prow = a.row_of[el];
    }
    const double zfv = wi.zf[wi.f];
    const bool okl = zfv == wi.zf[wi.bx * RTUS_BLOCK] && isfinite(xf);
    const bool okw = !__builtin_amdgcn_ballot_w64(!okl);
    double lo = 0.0, hi = 0.0;
    if (okw) { lo = wave_min_f64(xf); hi = wave_max_f64(xf); }           // (wave-uniform: random targets pay the load and the ballot only)
    if ((threadIdx.x & 63) == 0) { const int w = threadIdx.x >> 6; hdr.flo[w] = lo; hdr.fhi[w] = hi; hdr.fok[w] = okw; }
    if (first_wave) {
        const int lane = threadIdx.x;
        const bool in = lane < wi.ne;
        const double zfirst = __shfl(P.z0, 0);
        const bool oke = !__builtin_amdgcn_ballot_w64(in && !(P.z0 == zfirst && isfinite(P.x0)));
        const double elo = wave_min_f64(in ? P.x0 : (double)INFINITY), ehi = wave_max_f64(in ? P.x0 : -(double)INFINITY);
        if (lane == 0) { hdr.elo = elo; hdr.ehi = ehi; hdr.ze = zfirst; hdr.eok = oke; }
        rec[lane].xe = P.x0;
        if (PERM) rec[lane].row = prow;
    }
    return zfv;
}

// Behind the barrier: what the waves left says whether the workgroup is eligible (wave-uniform)
__device__ __forceinline__ bool rowtab_eligible(const RowTabHdr& hdr)
{
    return __builtin_amdgcn_readfirstlane(hdr.fok[0] & hdr.fok[1] & hdr.fok[2] & hdr.fok[3] & hdr.eok);
}

// The lattice of an eligible workgroup, from the header (wave-uniform).  fits: the span is within the capacity.
struct RowTabLattice {
    double ze;                         // the elements' depth
    double h, inv_h, tlo;              // node X_j = j h; the table's first interval starts at node tlo
    int n_int;                         // intervals; nodes 0 .. n_int (<= the slots)
    bool fits;
};
__device__ __forceinline__ RowTabLattice rowtab_lattice(const RowTabHdr& hdr, double zfv)
{
    const double zE = hdr.ze, D = zfv - zE, elo = hdr.elo, ehi = hdr.ehi;
    const double flo = fmin(fmin(hdr.flo[0], hdr.flo[1]), fmin(hdr.flo[2], hdr.flo[3]));
    const double fhi = fmax(fmax(hdr.fhi[0], hdr.fhi[1]), fmax(hdr.fhi[2], hdr.fhi[3]));
    const double gap = fmax(fmax(flo - ehi, elo - fhi), 0.0), far = fmax(fhi - elo, ehi - flo);
    const double h = __longlong_as_double(__double_as_longlong(D * RTUS_ROWTAB_DIV) & 0x7ff0000000000000ll);
    const double inv_h = __longlong_as_double(0x7fe0000000000000ll - __double_as_longlong(h));      // exact: h is a power of two
    const double tlo = floor(gap * inv_h), thi = floor(far * inv_h);
    // (D > 0 is zf > ze; the limits keep h and 1 / h normal and the indices in an int; NaN fails every comparison)
    const bool fits = D > 1e-290 && D < 1e290 && thi < 1073741824.0 && thi - tlo < (double)(RTUS_ROWTAB_SLOTS - 1);
    return {zE, h, inv_h, tlo, __builtin_amdgcn_readfirstlane(fits ? (int)(thi - tlo) : 0) + 1, __builtin_amdgcn_readfirstlane((int)fits) != 0};
}

// The build: the node pass, the interval pass with its check, the workgroup's vote.  Returns whether the workgroup serves.
template <int NL>
__device__ __forceinline__ bool rowtab_build(const LayerArgs& a, const WorkItem& wi, const RowTabLattice& lat, RowTabSlot* tab,
                                             RowTabHdr& hdr, double& xf)
{
    const double h = lat.h, tlo = lat.tlo;
    const int n_int = lat.n_int;
    const int tid = threadIdx.x, w0 = __builtin_amdgcn_readfirstlane(tid) & ~63;
    Lane<NL> LT;
    layer_setup<NL>(a, lat.ze, wi.zf, wi.f8, LT);
    bool bad = false;
    for (int base = w0; base <= n_int; base += RTUS_BLOCK) {                     // (wave-uniform: a wave without a node skips)
        const int k = min(base + (tid & 63), n_int);
        double T, p, pp;
        bad |= !rowtab_point<NL>(LT, (tlo + (double)k) * h, T, p, pp);
        tab[k].c[0] = T; tab[k].c[1] = p * h; tab[k].c[2] = pp * (0.5 * h * h);   // (lanes past the last node redo it: same values)
    }
    __syncthreads();
    RTUS_STAMP(2);
    for (int base = w0; base < n_int; base += RTUS_BLOCK) {
        const int j = min(base + (tid & 63), n_int - 1);
        double Tc, pc, ppc;                                                      // (the solve first: the coefficients are not live across it)
        const bool okc = rowtab_point<NL>(LT, ((tlo + (double)j) + RTUS_ROWTAB_CHECK_S) * h, Tc, pc, ppc);
        const double c0 = tab[j].c[0], c1 = tab[j].c[1], c2 = tab[j].c[2];
        const double d = ((tab[j + 1].c[0] - c0) - c1) - c2, e = (tab[j + 1].c[1] - c1) - 2.0 * c2, g = 2.0 * (tab[j + 1].c[2] - c2);
        const double c3 = fma(10.0, d, fma(-4.0, e, 0.5 * g)), c4 = fma(-15.0, d, fma(7.0, e, -g)), c5 = fma(6.0, d, fma(-3.0, e, 0.5 * g));
        // (the upper three: words no node pass wrote and no other lane reads now — no barrier between the reads and these)
        tab[j].c[3] = c3; tab[j].c[4] = c4; tab[j].c[5] = c5;
        const double sc = RTUS_ROWTAB_CHECK_S;
        const double Ti = fma(sc, fma(sc, fma(sc, fma(sc, fma(sc, c5, c4), c3), c2), c1), c0);
        bad |= !(okc && fabs(Ti - Tc) <= RTUS_ROWTAB_BOUND * Tc);
    }
    // (the target's x is LOADED again here — an L2 hit, through an offset the compiler cannot see through, as layer_setup
    // does with zf — instead of being held across the build, which has no register to spare for it: two went to scratch)
    unsigned f8r = wi.f8;
    asm volatile("" : "+v"(f8r));
    xf = *(const double*)((const char*)wi.xf + f8r);
    const bool badw = __builtin_amdgcn_ballot_w64(bad) != 0;
    if ((tid & 63) == 0) hdr.bad[tid >> 6] = badw;
    __syncthreads();
    RTUS_STAMP(3);
    return !__builtin_amdgcn_readfirstlane(hdr.bad[0] | hdr.bad[1] | hdr.bad[2] | hdr.bad[3]);
}

// Serving: a row per trip (wave-uniform), every lane its own target.
template <bool PERM>
__device__ __forceinline__ void rowtab_serve(const WorkItem& wi, const RowTabLattice& lat, const RowTabSlot* tab, const RowDest<PERM>& dest,
                                             double xf)
{
    // the rows leave WRITE-THROUGH (sc1, the store's cache-policy operand 16): a table that takes this path is larger than
    // the L2s together, so a line kept there serves nobody and is only written back later, at the launch's end at the latest
    constexpr int store_policy = 16;
    const RecPtr rec3 = (RecPtr)dest.rec;
    const double inv_h = lat.inv_h, tlo = lat.tlo;
    size_t ot = dest.o0;
    unsigned sot = 0;
    for (int l = 0; l < wi.ne; ++l) {
        const double tq = fma(fabs(xf - rec3[l].xe), inv_h, -tlo);              // X / h - tlo, exact
        const double sq = __builtin_amdgcn_fract(tq);
        const RowTabSlot* __restrict__ sl = &tab[(int)tq];
        const double T = fma(sq, fma(sq, fma(sq, fma(sq, fma(sq, sl->c[5], sl->c[4]), sl->c[3]), sl->c[2]), sl->c[1]), sl->c[0]);
        const u32x2 bits = {(unsigned)__double2loint(T), (unsigned)__double2hiint(T)};
        if (l == 0) RTUS_STAMP(4);                                               // (nothing in a product build)
        __builtin_amdgcn_raw_buffer_store_b64(bits, dest.rsrc(l, ot), wi.f8, dest.soff(sot), store_policy);
        ot += dest.nf; sot += dest.row_bytes;
    }
}

// ---- the solver over the block -----------------------------------------------------------------------------------------------
template <int V> struct HoldMode { static constexpr int value = V; };

template <int NL, bool ITERS, bool TAUP, bool PERM>
__device__ __forceinline__ void solve_block(const LayerArgs& a, const WorkItem& wi, double xf, const RowDest<PERM>& dest)
{
#ifdef RTUS_EXP_NO_HOLD                                     // experiment builds only (scripts/build_variant.sh nohold): every solve forms its own X' and u^3
    constexpr bool HOLDS = false;
#else
    constexpr bool HOLDS = TAUP;
#endif
    const ElemRec* rec = dest.rec;
    const RecPtr rec3 = (RecPtr)rec;
    uint8_t* __restrict__ it_p = wi.iters;
    const unsigned f8 = wi.f8;
    const bool live = wi.live;
    const size_t nf = dest.nf;
    const unsigned row_bytes = dest.row_bytes;
    size_t o = dest.o0;                                      // output row of element e0 + li (wave-uniform; ITERS only)
    unsigned so = 0;                                         // li * row_bytes
    int li = 0;
    Lane<NL> L;
    L.tau = INFINITY; L.rS3 = 0.0f; L.G = L.dG = 0.0f; L.hic = 0.0f; L.inv_cm = 0.0; L.hr0 = L.hc0 = 0.0; L.hr0f = L.rs0f = L.rhmf = L.asymf = 0.0f;
#pragma unroll
    for (int i = 0; i < NL; ++i) { L.hr[i] = L.kk[i] = L.hc[i] = 0.0; L.hrf[i] = L.kkf[i] = 0.0f; }
    float qa = 0.0f, qb = 0.0f, qc = 0.0f, qd = 0.0f;       // signed solutions of the four previous elements, qa the latest
    while (li < wi.ne) {                                     // wave-uniform loop
        const int info = __builtin_amdgcn_readfirstlane(rec[li].info);
        if (info & 8) {                                      // depth changed: redo the layer set-up, forget the history
            layer_setup<NL>(a, wi.ze[wi.e0 + li], wi.zf, f8, L);
            qa = qb = qc = qd = 0.0f;                        // a lane may carry NaN history from a depth at which its target
                                                             // was not below the element
        }
        const int run4 = (info >> 8) & ~3;
        if (run4 > 0) {
            // four-history run, unrolled by four so that the history rotates through its registers without moves.  The records are
            // read at ONE per-lane address register advanced once per trip, with immediate offsets (left to itself the compiler
            // forms each record's address on the scalar unit and pays a v_mov per ds_read: two VALU slots per solve)
            unsigned rp_off = (unsigned)li * (unsigned)sizeof(ElemRec);
            asm volatile("" : "+v"(rp_off));
            RecPtr rp = (RecPtr)((const __attribute__((address_space(3))) char*)rec3 + rp_off);
            // the group of four at rows i .. i + 3 of the block, in two pieces: its first solve, and the other three
            auto first = [&](auto hold, int i, bool after_held, bool* ok) {
                qd = solve_elem<NL, ITERS, true, TAUP, decltype(hold)::value>(it_p, L, rp + 0, 4, xf, qa, qb, qc, qd, live, dest.row(i, o), f8, dest.rsrc(i, o), dest.soff(so), after_held, ok);
            };
            auto others = [&](auto hold, int i) {
                qc = solve_elem<NL, ITERS, true, TAUP, decltype(hold)::value>(it_p, L, rp + 1, 4, xf, qd, qa, qb, qc, live, dest.row(i + 1, o + nf), f8, dest.rsrc(i + 1, o + nf), dest.soff(so + row_bytes));
                qb = solve_elem<NL, ITERS, true, TAUP, decltype(hold)::value>(it_p, L, rp + 2, 4, xf, qc, qd, qa, qb, live, dest.row(i + 2, o + 2 * nf), f8, dest.rsrc(i + 2, o + 2 * nf), dest.soff(so + 2 * row_bytes));
                qa = solve_elem<NL, ITERS, true, TAUP, decltype(hold)::value>(it_p, L, rp + 3, 4, xf, qb, qc, qd, qa, live, dest.row(i + 3, o + 3 * nf), f8, dest.rsrc(i + 3, o + 3 * nf), dest.soff(so + 3 * row_bytes));
            };
            // HOLD (tau-p tier).  The untaken Newton step dq = dXf / X' and the tail's second-order term G dXf^2 need X'(q) and u^3
            // only to a few per cent — dq moves the history by <= tau q, the term is <= (tau^2 / 8) T — and both drift by ~1-2 % from
            // one element to the next.  So the FIRST solve of a group of four forms them exactly (HOLD = 1: the sum for X', v_rcp_f32,
            // u^3) and, where the root moves by <= 0.02 per element (wave-uniform test: the curvature of G bounds the secant through
            // the last two exactly formed G to within 8.4 % of G over three elements, see HOLD = 1) and the pitch is uniform around the
            // group (bit 4 of the record: the secant runs along the element index), the other three reuse them (HOLD = 2: eleven fp32
            // instructions fewer per solve, stopping at tau / 3); otherwise they form their own (HOLD = 0).  Error of the held term:
            // <= 8.4 % of ((tau / 3)^2 / 8) T = 1.05e-10 T at the stopping threshold, 1e-15 T typically; with the fp32 residual's
            // (tau / 3) 2e-7 T a held solve is within 1.25e-10 T.
            // A row's bits stay a function of the table (the groups start where the four-history run starts: a function of the
            // aperture and of the rows per block).
            bool held = false;                              // the previous group of this run was held: L.G is extrapolated (see HOLD = 1)
            for (int r = 0; r < run4; r += 4) {
                if (HOLDS) {
                    bool ok = false;
                    first(HoldMode<HOLDS ? 1 : 0>{}, li + r, held, &ok);
                    if (ok) others(HoldMode<HOLDS ? 2 : 0>{}, li + r);
                    else others(HoldMode<0>{}, li + r);
                    held = ok;
#ifdef RTUS_EXP_COUNT   // groups of four, and how many of them reused the first solve's X' and u^3
                    if ((threadIdx.x & 63) == 0) { atomicAdd(&planar_dbg[5], 1ull); if (ok) atomicAdd(&planar_dbg[6], 1ull); }
#endif
                } else {
                    first(HoldMode<0>{}, li + r, false, nullptr);
                    others(HoldMode<0>{}, li + r);
                }
                o += 4 * nf; so += 4 * row_bytes;
                rp += 4;
            }
            li += run4;
        } else {
            const float qn = solve_elem<NL, ITERS, false, TAUP>(it_p, L, rec3 + li, info & 7, xf, qa, qb, qc, qd, live, dest.row(li, o), f8, dest.rsrc(li, o), dest.soff(so));
            qd = qc; qc = qb; qb = qa; qa = qn;
            o += nf; so += row_bytes;
            ++li;
        }
    }
}

// NL = number of layers the medium has (n_if + 1); TAUP: the tau-p tail (accuracy tier); PERM: the elements arrive sorted by
// (depth, position) and element i's row of the table is a.row_of[i] — an aperture handed over in any order gets the predictor.
template <int NL, bool ITERS, bool TAUP = false, bool PERM = false>
__global__ __launch_bounds__(RTUS_BLOCK, (NL <= 3 && !ITERS) ? 8 : 1) void rtus_tt_layers_kernel(LayerArgs a)
{
    __shared__ ElemRec rec[64];
#ifdef RTUS_EXP_NO_ROWTAB                                   // experiment builds only: the solver path everywhere
    constexpr bool ROWTAB = false;
#else
    constexpr bool ROWTAB = TAUP && !ITERS;                  // the row table is a path of the tau-p tier (see rowtab_point)
#endif
    // the table itself is DYNAMIC LDS, asked for by launch_layers only where a block can qualify (a.rowtab): a table of short blocks
    // — configs[1], configs[4] — launches with the 2 KB of records it always had
    extern __shared__ __attribute__((aligned(16))) RowTabSlot tab[];
    __shared__ RowTabHdr hdr;
    const WorkItem wi = work_item<ITERS, ROWTAB>(a);
    double xf = wi.xf[wi.f];
    RTUS_STAMP(0);
    const bool first_wave = threadIdx.x < 64;
    const int el = min(wi.e0 + (int)(threadIdx.x & 63), a.n_e - 1);   // the first wave: its lane's element
    double zfv = 0.0;
    if (wi.try_tab) zfv = rowtab_ranges<PERM>(a, wi, xf, el, rec, hdr);
    else if (first_wave) solver_records<TAUP, PERM>(a, wi, el, rec);
    __syncthreads();
    RTUS_STAMP(1);
    const RowDest<PERM> dest = row_dest<PERM>(a, wi, rec);
    if (wi.try_tab) {
        if (rowtab_eligible(hdr)) {
            const RowTabLattice lat = rowtab_lattice(hdr, zfv);
            if (lat.fits && rowtab_build<NL>(a, wi, lat, tab, hdr, xf)) {
                rowtab_serve<PERM>(wi, lat, tab, dest, xf);
                RTUS_STAMP(5);
                return;
            }
        }
        // The workgroup tried the table and does not serve from it (ineligible, too wide a span, a rejected build): the solver needs
        // the full records now.  Every wave arrives here together (the decisions above are the workgroup's), none has read a record.
        if (first_wave) solver_records<TAUP, PERM>(a, wi, el, rec);
        __syncthreads();
    }
    solve_block<NL, ITERS, TAUP, PERM>(a, wi, xf, dest);
}

// Order of the aperture.  The predictor extrapolates from the four previous elements of a workgroup's block, which only works when
// consecutive elements are neighbours in space at one depth; an aperture handed over in another order fell back to cold-started
// Newton (~4.5 evaluations instead of 1).  rtus_rank_kernel sorts it by (depth, position, index) — every element counts the
// elements before it in that order (O(n^2) compares, a wave per element: 65 k for 256 elements) and drops its coordinates and its
// index at that rank — and the PERM kernels store each row where it belongs.  Keys are the IEEE bits made monotone, so the order
// is total whatever the values.
__device__ __forceinline__ unsigned long long order_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__global__ __launch_bounds__(256) void rtus_rank_kernel(const double* __restrict__ xe, const double* __restrict__ ze, int n,
                                                        double* __restrict__ xs, double* __restrict__ zs, int* __restrict__ row_of)
{
    // one WAVE per element: 64 compares per step, a ballot count each (a thread per element looping over all the others is a
    // chain of n dependent steps on one wave: 33 us for 256 elements)
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;                                       // wave-uniform
    const double x = xe[i], z = ze[i];
    const unsigned long long mx = order_key(x), mz = order_key(z);
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + lane;
        const unsigned long long ox = order_key(xe[min(j, n - 1)]), oz = order_key(ze[min(j, n - 1)]);
        const bool before = j < n && ((oz < mz) || (oz == mz && (ox < mx || (ox == mx && j < i))));
        rank += __popcll(__ballot(before));
    }
    if (lane == 0) { xs[rank] = x; zs[rank] = z; row_of[rank] = i; }
}

// Elements (table rows) per workgroup: as many as possible (predictor + set-up reuse: the first four elements of a workgroup
// start Newton cold) while keeping >= ~4 waves per SIMD; 64 once that still leaves two full rounds of 8 waves per SIMD (measured
// on BASELINE config 3: 32 -> 64 elements per workgroup = -4.5 % time; on config 2: 8 is the optimum).  A function of the
// WHOLE table (n_rows_total x n_f, x n_batch problems), never of the launch: row shards of a table use the table's value.
int rtus_rows_per_block(long long n_rows_total, int n_f, int n_batch, int elem_bytes)
{
    const long long wave_solves = (long long)((n_f + 63) / 64) * n_rows_total * n_batch;
    int eb = (int)(wave_solves / (1024LL * 4));
    eb = eb < 1 ? 1 : (eb > 32 ? 32 : eb);
    if (wave_solves >= 1024LL * 16 * 64) eb = 64;
    // fp32 tables are the curved-lens kernel's (the planar kernel is fp64 only): its block starts with three cold solves (~490 of
    // a 64-row block's 3,600 VALU instructions once most rows need no Newton step), so twice the rows per block where that still
    // leaves two full rounds of waves
    const int eb_max = elem_bytes == 4 ? 128 : 64;
    if (elem_bytes == 4 && wave_solves >= 1024LL * 16 * 128) eb = 128;
#ifdef RTUS_EXP_EB                                          // experiment builds only (scripts/ab_planar.py)
    eb = RTUS_EXP_EB < 1 ? 1 : (RTUS_EXP_EB > eb_max ? eb_max : RTUS_EXP_EB);
#endif
    while ((n_rows_total + eb - 1) / eb > 65535 && eb < eb_max) ++eb;   // grid.y limit (eb <= 64 / 128: one LDS record per element)
    if ((unsigned long long)eb * (unsigned long long)n_f * (unsigned)elem_bytes >= 0xffffffffull)   // row offsets inside a block are 32-bit
        eb = (int)(0xffffffffull / ((unsigned long long)n_f * (unsigned)elem_bytes));
    return eb;
}

// One launch of the instantiation that (iters, perm, taup) name, for a medium of NL layers
template <int NL>
static void launch_nl(bool iters, bool perm, bool taup, dim3 grid, dim3 block, unsigned lds, hipStream_t s, const LayerArgs& a)
{
    if (iters) hipLaunchKernelGGL((rtus_tt_layers_kernel<NL, true, false, false>), grid, block, lds, s, a);
    else if (perm && taup) hipLaunchKernelGGL((rtus_tt_layers_kernel<NL, false, true, true>), grid, block, lds, s, a);
    else if (perm) hipLaunchKernelGGL((rtus_tt_layers_kernel<NL, false, false, true>), grid, block, lds, s, a);
    else if (taup) hipLaunchKernelGGL((rtus_tt_layers_kernel<NL, false, true, false>), grid, block, lds, s, a);
    else hipLaunchKernelGGL((rtus_tt_layers_kernel<NL, false, false, false>), grid, block, lds, s, a);
}

static hipError_t launch_layers(const double* z_if, const double* c, int n_if, const double* xe, const double* ze, int n_e,
                                const double* xf, const double* zf, int n_f, double* tt, uint8_t* iters, int n_batch,
                                long long e_stride, long long f_stride, long long t_stride, int row0, long long n_rows_total,
                                unsigned flags, const int* row_of, hipStream_t s)
{
    LayerArgs a;
    a.row_of = row_of;
    for (int i = 0; i < RTUS_MAX_LAYERS; ++i) a.z_if[i] = i < n_if ? z_if[i] : INFINITY;
    for (int i = 0; i <= RTUS_MAX_LAYERS; ++i) { a.c[i] = i <= n_if ? c[i] : 1.0; a.inv_c[i] = 1.0 / a.c[i]; }
    a.n_if = n_if; a.xe = xe; a.ze = ze; a.xf = xf; a.zf = zf; a.tt = tt; a.iters = iters;
    a.n_e = n_e; a.n_f = n_f;
    a.e_stride = e_stride; a.f_stride = f_stride; a.t_stride = t_stride;
    const int eb = rtus_rows_per_block(n_rows_total, n_f, n_batch, 8);
    if (eb < 1 || (n_rows_total + eb - 1) / eb > 65535) return hipErrorInvalidValue;
    a.row0 = row0;
    a.eb = eb;
    a.n_rows = n_rows_total;
    a.rowtab = (flags & RTUS_TT_TAUP_TAIL) != 0 && !iters && eb >= RTUS_ROWTAB_MIN_ROWS;
    // work items: gx columns of 256 targets x gy blocks of rows (x n_batch problems), one workgroup each
    const int gx = (n_f + RTUS_BLOCK - 1) / RTUS_BLOCK;
    a.gy = (row0 + n_e - 1) / eb - row0 / eb + 1;
    if ((long long)gx * a.gy * n_batch > 0x7fffffffLL) return hipErrorInvalidValue;
    // (row-table launches: x and y flattened into grid.x, y fastest: see work_item; gx gy < 2^31, within grid.x's limit)
    const dim3 grid(a.rowtab ? gx * a.gy : gx, a.rowtab ? 1 : a.gy, n_batch), block(RTUS_BLOCK);
    const bool taup = (flags & RTUS_TT_TAUP_TAIL) != 0;
    // Workgroups per CU: what the registers allow (8 for the 64-VGPR kernels).  Capping a launch of two rounds or more BELOW that with
    // LDS the kernel never touches was worth -3.5 % at six per CU while the kernel still parked set-up values in scratch and loaded
    // extra header words (start-up that nothing overlapped when every wave of a SIMD began at once); on the kernel as it is now six
    // per CU is 0.5 - 1.6 % SLOWER than eight and seven is even: no shaping.
    const unsigned lds = a.rowtab ? (unsigned)(RTUS_ROWTAB_SLOTS * sizeof(RowTabSlot)) : 0u;
    switch (n_if + 1) {
        case 1: launch_nl<1>(iters != nullptr, row_of != nullptr, taup, grid, block, lds, s, a); break;
        case 2: launch_nl<2>(iters != nullptr, row_of != nullptr, taup, grid, block, lds, s, a); break;
        case 3: launch_nl<3>(iters != nullptr, row_of != nullptr, taup, grid, block, lds, s, a); break;
        case 4: launch_nl<4>(iters != nullptr, row_of != nullptr, taup, grid, block, lds, s, a); break;
        case 5: launch_nl<5>(iters != nullptr, row_of != nullptr, taup, grid, block, lds, s, a); break;
        case 6: launch_nl<6>(iters != nullptr, row_of != nullptr, taup, grid, block, lds, s, a); break;
        case 7: launch_nl<7>(iters != nullptr, row_of != nullptr, taup, grid, block, lds, s, a); break;
        case 8: launch_nl<8>(iters != nullptr, row_of != nullptr, taup, grid, block, lds, s, a); break;
        case 9: launch_nl<9>(iters != nullptr, row_of != nullptr, taup, grid, block, lds, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t rtus_launch_tt_layers(const double* z_if, const double* c, int n_if, const double* xe,
                                 const double* ze, int n_e, const double* xf, const double* zf, int n_f,
                                 double* tt, uint8_t* iters, unsigned flags, hipStream_t s)
{
    return launch_layers(z_if, c, n_if, xe, ze, n_e, xf, zf, n_f, tt, iters, 1, 0, 0, 0, 0, n_e, flags, nullptr, s);
}

// rows [row0, row0 + n_e) of a table of n_rows_total rows: the same bits as the whole table's launch gives those rows when
// row0 is a multiple of rtus_rows_per_block(n_rows_total, n_f, 1, 8)
hipError_t rtus_launch_tt_layers_rows(const double* z_if, const double* c, int n_if, const double* xe, const double* ze, int n_e,
                                      int row0, long long n_rows_total, const double* xf, const double* zf, int n_f, double* tt,
                                      unsigned flags, hipStream_t s)
{
    return launch_layers(z_if, c, n_if, xe, ze, n_e, xf, zf, n_f, tt, nullptr, 1, 0, 0, 0, row0, n_rows_total, flags, nullptr, s);
}

// n_batch independent problems of one shape and one medium in ONE launch (several apertures and / or target sets):
// problem b reads xe/ze + b e_stride, xf/zf + b f_stride and writes tt + b t_stride.
hipError_t rtus_launch_tt_layers_batch(const double* z_if, const double* c, int n_if, const double* xe, const double* ze,
                                       int n_e, long long e_stride, const double* xf, const double* zf, int n_f,
                                       long long f_stride, double* tt, long long t_stride, int n_batch, unsigned flags, hipStream_t s)
{
    return launch_layers(z_if, c, n_if, xe, ze, n_e, xf, zf, n_f, tt, nullptr, n_batch, e_stride, f_stride, t_stride, 0, n_e, flags, nullptr, s);
}

// The whole table with the aperture in ANY order: sorted copies of the coordinates + each element's row in `ws`
// (rtus_layers_sort_ws_bytes), then the PERM kernel.  `presorted_row_of`: the caller (the host-buffer twin) has sorted on the
// host and uploaded sorted xe / ze and the row indices itself — no rank launch.
struct SortWs { double* xs; double* zs; int* row_of; };
static size_t sort_ws(void* ws, int n_e, SortWs* w)         // the layout of `ws`, carved in ONE place: three 256-byte-aligned segments; returns its size
{
    const size_t seg = rtus_al256((size_t)n_e * 8);
    if (w) { w->xs = (double*)ws; w->zs = (double*)((char*)ws + seg); w->row_of = (int*)((char*)ws + 2 * seg); }
    return 2 * seg + rtus_al256((size_t)n_e * 4);
}
size_t rtus_layers_sort_ws_bytes(int n_e) { return sort_ws(nullptr, n_e, nullptr); }
hipError_t rtus_launch_tt_layers_sorted(const double* z_if, const double* c, int n_if, const double* xe, const double* ze, int n_e,
                                        const double* xf, const double* zf, int n_f, double* tt, void* ws, const int* presorted_row_of,
                                        unsigned flags, hipStream_t s)
{
    if (presorted_row_of)
        return launch_layers(z_if, c, n_if, xe, ze, n_e, xf, zf, n_f, tt, nullptr, 1, 0, 0, 0, 0, n_e, flags, presorted_row_of, s);
    SortWs w;
    sort_ws(ws, n_e, &w);
    hipLaunchKernelGGL(rtus_rank_kernel, dim3((n_e + 3) / 4), dim3(256), 0, s, xe, ze, n_e, w.xs, w.zs, w.row_of);
    return launch_layers(z_if, c, n_if, w.xs, w.zs, n_e, xf, zf, n_f, tt, nullptr, 1, 0, 0, 0, 0, n_e, flags, w.row_of, s);
}

// ---- Matrix arrays: elements (xe, ye, ze) x points (xf, yf, zf) ---------------------------------------------------------------
// Horizontal layers are symmetric about the vertical axis: the ray from an element to a point lies in the vertical plane through
// both, and its time is the planar time at lateral reach r = sqrt(dx dx + dy dy), dx = xf - xe, dy = yf - ye, between the depths ze
// and zf.  The mathematics is the planar solver's (layer_setup, the fp32 Newton loop clamped to the root's lower bound, the fp64
// tail with the second-order Fermat term); none of its speed machinery carries over — the predictor along a linear aperture, HOLD
// and the row table all lean on xf - xe being signed and linear along the element index.
// EVERY SOLVE STARTS COLD, from the lower bound that its own reach gives: nothing is carried from element to element, so the bits of
// tt[e][f] are a function of the pair (and the medium) alone — not of the order of the elements or points, of what else the call
// holds, or of how a table is cut into calls.  (A lane that is done does not take its step and re-derives the same dq while its
// wave goes on: the wave's trip count does not reach the bits.  layer_setup is a pure function of (ze, zf): re-using it while the
// depth repeats gives what running it again gives.)
// Launch shape: a workgroup = RTUS_TT_LAYERS3_POINTS points (one per lane: a row's stores are contiguous) x RTUS_TT_LAYERS3_ROWS
// consecutive elements (loop); the elements' coordinates sit in LDS and are broadcast.  Work items are flattened into grid.x, the
// columns of points fastest.
static_assert(RTUS_TT_LAYERS3_POINTS == RTUS_BLOCK, "one point per lane of the workgroup");

struct Layers3Args {
    LayerArgs a;                       // the medium, xe / ze / xf / zf / tt, n_e, n_f (the planar launch's fields are unused)
    const double* __restrict__ ye;
    const double* __restrict__ yf;
    int gx;                            // columns of points
};

// The travel time at reach X >= 0 through the lane's layers: Newton from the lower bound of the root (solve_elem's cold start), then
// the default tier's tail.  A function of (X, L) alone.
template <int NL>
__device__ __forceinline__ double solve_reach(const Lane<NL>& L, double X)
{
    const float Xf = (float)X;
    const float lb = fmaxf(fmaxf(Xf * L.rs0f, (Xf - L.asymf) * L.rhmf), 0.0f);
    float q = lb, y[NL], rS3 = 0.0f;
    for (int trip = 0; trip < 64; ++trip) {                 // wave-uniform trip count, ballot exit
        const float q2 = q * q;
        float S1 = L.hr0f, S3 = L.hr0f;                     // slot 0: k = 0, y = 1
#pragma unroll
        for (int i = 1; i < NL; ++i) {
            y[i] = __builtin_amdgcn_rsqf(fmaf(L.kkf[i], q2, 1.0f));
            const float hw = L.hrf[i] * y[i];
            S1 += hw;
            S3 = fmaf(hw, y[i] * y[i], S3);
        }
        rS3 = __builtin_amdgcn_rcpf(S3);
        const float dq = fmaf(-S1, q, Xf) * rS3;
        const bool big = fabsf(dq) > L.tau * q;             // tau = +inf on lanes without a path, NaN on a non-finite reach: never a step
        if (!__builtin_amdgcn_ballot_w64(big)) break;
        q = big ? fmaxf(q + dq, lb) : q;                    // a lane that is done keeps its q: y[] and rS3 stay those of its q
    }
    // T(root) = T(q) + p dXr + (1/2) (dp/dX) dXr^2 + O(dXr^3), dXr = X - X(q) in fp64: see solve_elem
    const double qd = (double)q, q2 = qd * qd, a1 = 1.0 + q2;
    const float us = __builtin_amdgcn_rsqf(fmaf(q, q, 1.0f));
    const double u = rsqrt_refine(a1, (double)us);
    double A1 = L.hr0, ST = L.hc0;
#pragma unroll
    for (int i = 1; i < NL; ++i) {
        const double w = rsqrt_refine(fma(L.kk[i], q2, 1.0), (double)y[i]);
        A1 = fma(L.hr[i], w, A1);
        ST = fma(L.hc[i], w, ST);
    }
    const double dXr = fma(-A1, qd, X);
    const float s2 = (0.5f * us) * (us * rS3);
    return u * fma(L.inv_cm, dXr * fma((double)s2, dXr, qd), a1 * ST);
}

template <int NL>
__global__ __launch_bounds__(RTUS_BLOCK) void rtus_tt_layers3_kernel(Layers3Args g)
{
    __shared__ double ex[RTUS_TT_LAYERS3_ROWS], ey[RTUS_TT_LAYERS3_ROWS], ez[RTUS_TT_LAYERS3_ROWS];
    const LayerArgs& a = g.a;
    const int bx = (int)(blockIdx.x % (unsigned)g.gx), by = (int)(blockIdx.x / (unsigned)g.gx);
    const int e0 = by * RTUS_TT_LAYERS3_ROWS, ne = min(RTUS_TT_LAYERS3_ROWS, a.n_e - e0);
    if ((int)threadIdx.x < ne) {
        ex[threadIdx.x] = a.xe[e0 + threadIdx.x];
        ey[threadIdx.x] = g.ye[e0 + threadIdx.x];
        ez[threadIdx.x] = a.ze[e0 + threadIdx.x];
    }
    // lanes beyond the last point redo the last one and store to its address: no index leaves the buffers
    const int f = min(bx * RTUS_BLOCK + (int)threadIdx.x, a.n_f - 1);
    const unsigned f8 = (unsigned)f * 8u;                   // (n_f < 2^29: the launcher checks)
    const double xf = a.xf[f], yf = g.yf[f];
    __syncthreads();
    const unsigned row_bytes = (unsigned)a.n_f * 8u;
    double* __restrict__ row = a.tt + (size_t)e0 * (size_t)a.n_f;   // 64-bit: n_e n_f 8 passes 4 GiB at production sizes
    Lane<NL> L;
    for (int i = 0; i < ne; ++i, row += a.n_f) {
        const double ze = ez[i];
        // the layer table depends on (ze, zf): a flat matrix array sets up once per lane (wave-uniform: the depths are the block's)
        if (i == 0 || __builtin_amdgcn_readfirstlane((int)!(ze == ez[i - 1]))) {
            layer_setup<NL>(a, ze, a.zf, f8, L);
            // a depth that is not finite has no path (layer_setup knows zf <= ze and NaN, not +-inf)
            L.hc0 = isfinite(a.zf[f] - ze) ? L.hc0 : NAN;
        }
        const double dx = xf - ex[i], dy = yf - ey[i];
        const double r = sqrt(dx * dx + dy * dy);           // IEEE: correctly rounded (-fno-fast-math); dy = 0: |dx| exactly
        double T = solve_reach<NL>(L, r);
        T = isfinite(r) ? T : NAN;
        // one descriptor per row (extent: the row), each lane a 32-bit byte offset inside it
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(row, 0, row_bytes, 0x00020000);
        const u32x2 bits = {(unsigned)__double2loint(T), (unsigned)__double2hiint(T)};
        __builtin_amdgcn_raw_buffer_store_b64(bits, rs, f8, 0, 0);
    }
}

hipError_t rtus_launch_tt_layers3(const double* z_if, const double* c, int n_if, const double* xe, const double* ye, const double* ze,
                                  int n_e, const double* xf, const double* yf, const double* zf, int n_f, double* tt, hipStream_t s)
{
    Layers3Args g = {};
    LayerArgs& a = g.a;
    for (int i = 0; i < RTUS_MAX_LAYERS; ++i) a.z_if[i] = i < n_if ? z_if[i] : INFINITY;
    for (int i = 0; i <= RTUS_MAX_LAYERS; ++i) { a.c[i] = i <= n_if ? c[i] : 1.0; a.inv_c[i] = 1.0 / a.c[i]; }
    a.n_if = n_if; a.xe = xe; a.ze = ze; a.xf = xf; a.zf = zf; a.tt = tt; a.n_e = n_e; a.n_f = n_f;
    g.ye = ye; g.yf = yf;
    g.gx = (n_f + RTUS_BLOCK - 1) / RTUS_BLOCK;
    const long long wgs = (long long)g.gx * ((n_e + RTUS_TT_LAYERS3_ROWS - 1) / RTUS_TT_LAYERS3_ROWS);
    if (n_f >= (1 << 29) || wgs > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)wgs), block(RTUS_BLOCK);
    switch (n_if + 1) {
        case 1: hipLaunchKernelGGL(rtus_tt_layers3_kernel<1>, grid, block, 0, s, g); break;
        case 2: hipLaunchKernelGGL(rtus_tt_layers3_kernel<2>, grid, block, 0, s, g); break;
        case 3: hipLaunchKernelGGL(rtus_tt_layers3_kernel<3>, grid, block, 0, s, g); break;
        case 4: hipLaunchKernelGGL(rtus_tt_layers3_kernel<4>, grid, block, 0, s, g); break;
        case 5: hipLaunchKernelGGL(rtus_tt_layers3_kernel<5>, grid, block, 0, s, g); break;
        case 6: hipLaunchKernelGGL(rtus_tt_layers3_kernel<6>, grid, block, 0, s, g); break;
        case 7: hipLaunchKernelGGL(rtus_tt_layers3_kernel<7>, grid, block, 0, s, g); break;
        case 8: hipLaunchKernelGGL(rtus_tt_layers3_kernel<8>, grid, block, 0, s, g); break;
        case 9: hipLaunchKernelGGL(rtus_tt_layers3_kernel<9>, grid, block, 0, s, g); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
