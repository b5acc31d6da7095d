/*
 * rtus.h — C ABI of librtus.so, the MI355X (gfx950) travel-time ray tracer.
 *
 * This is the drop-in boundary for ONE hot path of edudscrc/ray-tracing-ultrasound: the
 * ray-tracing loop of main_rt.py (shoot_rays + element matcher) and the element x focal-point
 * travel-time solves built on it.  The reference has no FFI of its own — its boundary is the
 * Python function shoot_rays(x_a, z_a, z_f, alpha, plot) -> dict of 8 float64[N]
 * (main_rt.py:337, 432-441) plus module globals (main_rt.py:449-467).  Every entry point below
 * names the reference lines it replaces; INTEGRATION.md shows the ctypes stub a maintainer adds.
 *
 * Conventions
 *   - plain C: pointers + sizes, no C++/torch types; all functions return 0 (RTUS_OK) or a
 *     negative rtus_status; nothing throws.  The "*_dev" entry points keep no state and are re-entrant per
 *     (device, stream).  The host-buffer twins keep ONE thing: a per-device staging arena (a grow-only device
 *     allocation + a non-blocking stream, created on first use, freed by rtus_release) — the reference's calling
 *     pattern is hundreds of small sequential calls (main_rt.py:464-482), and a hipMalloc per buffer and call cost
 *     more than the kernels.  Host-buffer calls on one device are serialised by that arena's lock.
 *   - all real data is float64 unless the name ends in _f32.
 *   - "*_dev" entry points take DEVICE pointers and a hipStream_t (passed as void*), launch
 *     asynchronously and never allocate or synchronise.  The un-suffixed twins take HOST
 *     buffers, stage them through HBM on `device`, run the same kernels and synchronise.
 *   - invalid rays are NaN (never sentinels), exactly as the reference's consumers expect
 *     (main_compare.py:531-534, main_rt.py:495).
 */
#ifndef RTUS_H
#define RTUS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTUS_VERSION 127 /* 0.1.26: rtus_tt_aniso_surface[_dev], rtus_tt_aniso_direct[_dev] (travel times into an anisotropic part: the group slowness as a series in the ray angle) */

typedef enum rtus_status {
    RTUS_OK = 0,
    RTUS_ERR_INVALID_ARG = -1,   /* null pointer, non-positive size, bad flag (reference: ValueError main_rt.py:24-29) */
    RTUS_ERR_NO_DEVICE = -2,     /* no HIP device / device index out of range */
    RTUS_ERR_HIP = -3,           /* a HIP runtime call failed; rtus_last_hip_error() has the code */
    RTUS_ERR_WORKSPACE = -4,     /* workspace pointer null, not 64-byte aligned, or too small */
    RTUS_ERR_UNSUPPORTED = -5    /* e.g. more layers than RTUS_MAX_LAYERS */
} rtus_status;

/*
 * Acoustic-lens constants.  Replaces the module globals c1, c2, l0, h0, d that the reference's
 * helpers read implicitly (main_rt.py:181-201; set at main_rt.py:449-455).
 */
typedef struct rtus_lens {
    double c1; /* speed in the lens   [m/s]  main_rt.py:449 */
    double c2; /* speed in the water  [m/s]  main_rt.py:450 */
    double l0; /* lens design length  [m]    main_rt.py:453 */
    double h0; /* lens design height  [m]    main_rt.py:454 */
    double d;  /* array plane z = l0+h0 [m]  main_rt.py:455 */
} rtus_lens;

/* Slots of the 8-array result of shoot_rays (main_rt.py:432-441), in this order. */
enum {
    RTUS_LENS_1_X = 0, RTUS_LENS_1_Z = 1, RTUS_PIPE_X = 2, RTUS_PIPE_Z = 3,
    RTUS_LENS_2_X = 4, RTUS_LENS_2_Z = 5, RTUS_TARGET_X = 6, RTUS_TARGET_Z = 7
};

/* Per-ray status bits (optional output). */
#define RTUS_RAY_REF_RAISES 0x1u /* pipe point is NaN: the reference raises LinAlgError here (np.polyfit, main_rt.py:73); we return NaN */

const char *rtus_strerror(int status);
int rtus_version(void);
int rtus_last_hip_error(void);
int rtus_device_count(int *count);
/* Frees the host-buffer twins' staging arena of `device` (all devices: -1).  Optional: a process that exits without
 * calling it leaks nothing the driver does not reclaim. */
int rtus_release(int device);
/* Diagnostic (not in the reference): checks, on `device`, two facts the forward trace relies on — (a) its correctly
 * rounded division / square root sequences return the bits of a / b and sqrt(a) on n_math pseudo-random operand pairs
 * (exponents within +-500, every special value), (b) the depth-first bounding-box records of an n_rays-point lens
 * polyline form a tree (forward skip links that land where each box ends, leaves covering the polyline in order).
 * counts[0] = division mismatches, [1] = square-root mismatches, [2] = structure violations, [3] = n_math.  All zero
 * on a healthy build. */
/* Runs on `device` (validated; the caller's current device is restored) on the staging arena's own stream. */
int rtus_selftest(const rtus_lens *lens, int n_rays, long long n_math, unsigned long long *counts, int device);

/* ------------------------------------------------------------------------------------------
 * Forward trace — replaces shoot_rays (main_rt.py:337-405, 432-441) and its helpers
 * h_from_alpha/dh_from_alpha/x_z_from_alpha/dz_dx_from_alpha (:180-234), refraction/reflection
 * (:267-292), dzdx_pipe (:237-238), roots_bhaskara (:171-177) and the per-ray
 * find_line_curve_intersection loop (:6-168, :384-393), batched over n_geom pipe geometries
 * and n_tx transmit points.  Segment times replace dist + the TOF sums (main_rt.py:444-445,
 * 497-500; main_compare.py:514-517).
 *
 *   geoms   [n_geom][2]  (r_outer, pipe_offset)           main_rt.py:466-467
 *   x_a,z_a [n_tx]       transmit points                  main_rt.py:482
 *   alpha   [n_rays]     launch-angle grid; ALSO defines the lens polyline the reflected line is
 *                        intersected with (main_rt.py:338, 390)
 *   z_f     [n_rays]     landing plane per ray            main_rt.py:404
 *   out8    [n_geom][n_tx][8][n_rays]   nullable          main_rt.py:432-441
 *   tof4    [n_geom][n_tx][4][n_rays]   nullable          main_compare.py:514-517
 *   tof     [n_geom][n_tx][n_rays]      nullable  ((t1+t2)+t3)+t4, order of main_rt.py:497-500
 *   land_x  [n_geom][n_tx][n_rays]      nullable  (= out8 slot RTUS_TARGET_X alone)
 *   status  [n_geom][n_tx][n_rays]      nullable  RTUS_RAY_* bits
 * ---------------------------------------------------------------------------------------- */
/* flags for rtus_shoot*:
 *   0                     REFERENCE-COMPATIBLE.  What that means since round 3 (it is no longer the reference's angle chain
 *                         operation for operation):
 *                         - the reference's laws, quirks and decisions: chord polyline of the alpha grid (main_rt.py:385-390), pipe
 *                           tangent without the offset (:237-238, 367), lens root [1] / upper circle root (:187, 362-364), first sign
 *                           change in index order with np.sign(0) = 0 (:82-99), the +-1e-9 bounds check (:153-168), NaN for
 *                           total reflection and for |x_q| > r, no FMA contraction;
 *                         - formed AS THE REFERENCE FORMS THEM: the lens point and tangent (:180-234), the refracted angle
 *                           phi_pq = phi_s - pi/2 + asin(eta sin theta_1) and a = tan(phi_pq) (:267-280, 348: with the library's own
 *                           atan2 / sin / asin / tan where |a| > 300 — there the quadratic of :349-364 amplifies a last bit by |a|^3),
 *                           the circle intersection in slope-intercept form (:349-364), the chord intersection (:127-150), the landing
 *                           point (:402-404), the four segment times (:497-500), all with correctly rounded division / square root;
 *                         - formed ALGEBRAICALLY (the same real-number value, a few ulp from the reference's chain): sin theta_1 of the
 *                           entry refraction as a dot product of unit vectors; the reflected slope tan(2 atan(s) - phi_pq) as a rational
 *                           form in s's numerator and denominator (:283-292, 375); the exit refraction tan(phi_s - pi/2 + asin(eta
 *                           sin(...))) in vector form (:396-401) — total reflection is decided on eta sin theta_1 > 1 as in the reference,
 *                           but on a value ~1 ulp from its own, so a ray within a few ulp of the critical angle may be NaN on one side
 *                           and finite on the other (parity unpinned AT the critical angle; no golden ray sits there).
 *                         Guarantee, tested: NaN masks identical and every output within 1e-12 m / 1e-15 s on every golden captured from
 *                         the reference (tests/golden, the .npz files, 30 calls), database_2.csv's 13,650 flags and compare.csv's 1,810 rows
 *                         reproduced, and on random inputs |gpu - oracle| <= 1e-12 m + 16 x the oracle's OWN spread under 1-2 ulp
 *                         noise of its trigonometry (scripts/fuzz_shoot.py).  Measured on ill-conditioned rays (near-vertical lines,
 *                         grazing chords — the oracle moves as much under that noise): up to 8e-6 m from the oracle; and
 *                         tests/test_gpu_sweep_random_rows.py: the matcher's hit / first-ray decisions on 2,100 random rows outside
 *                         database_2.csv agree wherever the oracle keeps its own decision under that noise.
 *   RTUS_SHOOT_FAST_MATH  the same laws in vector form throughout (no trigonometry, reciprocal / rsqrt seeds + Newton): ~1e-15
 *                         relative from the above on regular rays, may differ on degenerate ones (exactly vertical / tangent rays). */
#define RTUS_SHOOT_FAST_MATH 0x1u
/* Physically-correct variants — these DEPART from the reference on purpose:
 *   RTUS_TRUE_PIPE_TANGENT  reflect on the tangent of the circle where it actually is; the reference evaluates
 *                           the tangent as if the pipe were centred at x = 0 (main_rt.py:237-238, 367)
 *   RTUS_ANALYTIC_LENS      intersect the reflected line with the analytic lens curve instead of the chords of
 *                           the alpha-grid polyline (main_rt.py:385-390) */
#define RTUS_TRUE_PIPE_TANGENT 0x2u
#define RTUS_ANALYTIC_LENS 0x4u
/* Device entry points only (the host-buffer twins ignore it): the workspace already holds the lens polyline of THIS alpha
 * grid, lens and n_rays — left there by a previous rtus_shoot_dev / rtus_solve_dev call on the same workspace — so the
 * call skips rebuilding it.  The polyline depends on nothing else (main_rt.py:338: x_p, z_p = x_z_from_alpha(alpha)), and
 * the reference's driver traces 210 geometries over one grid (main_rt.py:464-482). */
#define RTUS_POLYLINE_READY 0x8u

/* rtus_shoot (host buffers) keeps the lens polyline of its previous call on the device in a per-device arena and rebuilds it
 * only when alpha's VALUES or the lens constants differ from that call's (compared byte for byte) — the reference's script
 * calls shoot_rays 210 times over one grid (main_rt.py:464-482).  Invisible apart from the time it saves; rtus_release()
 * drops it.
 *
 * Device scratch of one call (polyline, tangents, bounding boxes and their depth-first records): 64-byte aligned
 * (hipMalloc gives 256), rebuilt by every call, not shared between calls that may run concurrently. */
size_t rtus_shoot_workspace_bytes(int n_rays);

int rtus_shoot_dev(const rtus_lens *lens, const double *d_geoms, int n_geom,
                   const double *d_x_a, const double *d_z_a, int n_tx,
                   const double *d_alpha, const double *d_z_f, int n_rays,
                   double *d_out8, double *d_tof4, double *d_tof, double *d_land_x,
                   uint8_t *d_status, void *d_workspace, size_t workspace_bytes, unsigned flags,
                   void *stream);

int rtus_shoot(const rtus_lens *lens, const double *geoms, int n_geom,
               const double *x_a, const double *z_a, int n_tx,
               const double *alpha, const double *z_f, int n_rays,
               double *out8, double *tof4, double *tof, double *land_x, uint8_t *status,
               unsigned flags, int device);

/* ------------------------------------------------------------------------------------------
 * Pulse-echo travel times by ROOT-FINDING: tx -> lens -> pipe -> lens -> rx with x_land(alpha) = x_rx solved
 * per (geometry, tx, rx element) — the north-star's replacement for the reference's grid scan
 * (main_rt.py:479-501: shoot a launch-angle grid, accept the first ray landing within atol of the element).
 * The ray chain is exactly rtus_shoot's (same flags); the alpha grid only brackets the roots and defines the
 * lens polyline.  x_land(alpha) is U-shaped: an element usually has two ray paths.
 *
 *   alpha [n_rays]  bracketing grid, STRICTLY ASCENDING = the lens polyline grid  main_rt.py:479, 338
 *                   (rtus_solve checks it: RTUS_ERR_INVALID_ARG; rtus_solve_dev cannot — device memory)
 *   x_rx  [n_rx]    receive elements on the plane z = z_land                     main_rt.py:469-477
 *   tt        [n_geom][n_tx][n_rx]      least travel time over the element's roots; NaN if none
 *   alpha_root[n_geom][n_tx][n_rx]      nullable: launch angle of that path
 *   tt_all, alpha_all [..][n_rx][RTUS_MAX_ROOTS]  nullable: every root in ascending alpha, NaN padded
 *   n_roots   [n_geom][n_tx][n_rx] uint8 nullable
 * Where the reference's scan reports a hit, one of the roots reproduces its tof to the scan's own resolution
 * (the hit ray lands up to atol + rtol|x| away from the element: <= ~3e-9 s, more at turning points of x_land).
 * ---------------------------------------------------------------------------------------- */
#define RTUS_MAX_ROOTS 4
/* How a bracket is refined depends on the SIZE of the call (a function of n_geom * n_tx * n_rx, nothing else): up to 32,768 (row,
 * element) pairs — the reference's own sweep has 13,650 — three lanes per bracket (the candidate and its two neighbours together:
 * two rounds of evaluations instead of two or three; such a call leaves most of the chip idle and lasts as long as its slowest
 * bracket), beyond that one lane per bracket.  Against a bisection to the last bit (scripts/fuzz_solve.py, 420 random trials, 82,472
 * roots, identical root counts): three lanes |dt| <= 8e-15 s, |dalpha| <= 1e-11 rad + the traces' own landing noise / slope; one
 * lane — it stops once the landing point is within 1e-9 m and its next step below 1e-8 rad, and applies that step — |dt| <= 6e-15 s,
 * |dalpha| <= 5e-11 rad + the same noise term (measured worst 1.9e-11 rad).  Within one scheme a bracket's bits do not
 * depend on the aperture's order or on the other brackets of the call.  RTUS_SOLVE_ONE_LANE asks for the one-lane scheme whatever
 * the size (bits independent of the call's size too). */
#define RTUS_SOLVE_ONE_LANE 0x10u
/* Such a small call with a grid of <= 1,024 rays and <= 128 elements (the reference's sweep: 905, 65) runs as ONE kernel after the
 * polyline's — a workgroup per (geometry, transmit point) row, landing points and pair masks in LDS.  RTUS_SOLVE_THREE_LAUNCHES
 * keeps the grid trace and the refinement as separate launches (the same bits: the refinement's arithmetic is one function). */
#define RTUS_SOLVE_THREE_LAUNCHES 0x20u
/* Which refinement a call of this size and these flags gets (host code, launches nothing; the launcher itself switches on it).
 * With rows = n_geom * n_tx and tasks = rows * n_rx:
 *   ROW         tasks <= 32,768, n_rays <= 1,024, n_rx <= 128, neither flag above: one kernel, a workgroup per row, three lanes per bracket
 *   TRIO_MASKS  tasks <= 32,768, n_rx <= 512, not ROW, no RTUS_SOLVE_ONE_LANE: separate launches, pair masks, three lanes per bracket
 *   TRIO_SCAN   tasks <= 32,768, n_rx > 512, no RTUS_SOLVE_ONE_LANE: the landing points are scanned in the kernel, three lanes per bracket
 *   HALF        n_rx <= 512, tasks <= 131,072 (and > 32,768, or RTUS_SOLVE_ONE_LANE): one lane per bracket, 128 element lanes per workgroup
 *   FULL        n_rx <= 512, tasks > 131,072: one lane per bracket, 256 element lanes per workgroup
 *   SCAN        n_rx > 512, tasks > 32,768 or RTUS_SOLVE_ONE_LANE: one lane per bracket, scanned landing points
 * -1: a size rtus_solve refuses (non-positive, n_rays < 2, or beyond its 2^31 limits). */
#define RTUS_SOLVE_PATH_ROW 0
#define RTUS_SOLVE_PATH_TRIO_MASKS 1
#define RTUS_SOLVE_PATH_TRIO_SCAN 2
#define RTUS_SOLVE_PATH_HALF 3
#define RTUS_SOLVE_PATH_FULL 4
#define RTUS_SOLVE_PATH_SCAN 5

size_t rtus_solve_workspace_bytes(int n_rays, int n_geom, int n_tx, int n_rx);
int rtus_solve_path(int n_geom, int n_tx, int n_rays, int n_rx, unsigned flags);

int rtus_solve_dev(const rtus_lens *lens, const double *d_geoms, int n_geom,
                   const double *d_x_a, const double *d_z_a, int n_tx,
                   const double *d_alpha, int n_rays, const double *d_x_rx, int n_rx, double z_land,
                   double *d_tt, double *d_alpha_root, double *d_tt_all, double *d_alpha_all,
                   uint8_t *d_n_roots, void *d_workspace, size_t workspace_bytes, unsigned flags,
                   void *stream);

int rtus_solve(const rtus_lens *lens, const double *geoms, int n_geom,
               const double *x_a, const double *z_a, int n_tx,
               const double *alpha, int n_rays, const double *x_rx, int n_rx, double z_land,
               double *tt, double *alpha_root, double *tt_all, double *alpha_all, uint8_t *n_roots,
               unsigned flags, int device);

/* ------------------------------------------------------------------------------------------
 * Element matcher — replaces the scan of main_rt.py:487-501: for each receive element the FIRST
 * ray (ascending index) with np.isclose(land_x[ray], x_rx[e], rtol, atol), i.e.
 * |land_x - x_rx| <= atol + rtol*|x_rx| for finite operands, land_x == x_rx when either is infinite,
 * never with a NaN (np.isclose's rules).  n_batch = n_geom*n_tx rows.
 * atol and rtol may be any values >= 0, rtol >= 1 included (there the fused sweep tests every element of an ascending chunk
 * instead of pruning it).  The decisions are np.isclose's to the last bit — atol + rtol*|x_rx| in two roundings, the difference
 * in one — also for landing points within an ulp of the tolerance's edge: what the kernels skip unseen is bounded by the
 * tolerance widened by a few ulp of its operands, never by a rounded x_rx +- tol alone (tests/test_gpu_match_edges.py).
 *
 *   land_x, tof [n_batch][n_rays]    (outputs of rtus_shoot*)
 *   x_rx        [n_rx]
 *   first_ray   [n_batch][n_rx] int32, -1 when no ray hits   (also the kernel's scratch)
 *   hit         [n_batch][n_rx] uint8  nullable               main_rt.py:496
 *   tof_hit     [n_batch][n_rx]        nullable, 0.0 if none  main_rt.py:493, 497-500
 * rtus_ray_hits: per ray, does ANY element match (main_compare.py:518-521).
 * ---------------------------------------------------------------------------------------- */
int rtus_match_dev(const double *d_land_x, const double *d_tof, int n_batch, int n_rays,
                   const double *d_x_rx, int n_rx, double atol, double rtol,
                   int32_t *d_first_ray, uint8_t *d_hit, double *d_tof_hit, void *stream);

int rtus_match(const double *land_x, const double *tof, int n_batch, int n_rays,
               const double *x_rx, int n_rx, double atol, double rtol,
               int32_t *first_ray, uint8_t *hit, double *tof_hit, int device);

int rtus_ray_hits_dev(const double *d_land_x, int n_batch, int n_rays, const double *d_x_rx,
                      int n_rx, double atol, double rtol, uint8_t *d_ray_hit, void *stream);

int rtus_ray_hits(const double *land_x, int n_batch, int n_rays, const double *x_rx, int n_rx,
                  double atol, double rtol, uint8_t *ray_hit, int device);

/* ------------------------------------------------------------------------------------------
 * Fused sweep — one body of the reference's parameter loop, main_rt.py:464-501: shoot_rays for every
 * (geometry, transmit element) row with the element matcher on its landing points inside the trace
 * kernel (the matcher runs on the landing points while they are still in registers; a small second
 * kernel turns the winners into first_ray / hit / tof_hit).  Results are bit-identical to rtus_shoot*
 * followed by rtus_match* on its land_x / tof outputs.
 *
 *   geoms, x_a, z_a, alpha, z_f, flags   as rtus_shoot*
 *   x_rx [n_rx], atol, rtol               as rtus_match*   (any n_rx; rows * (n_rx rounded up to 64) < 2^31)
 *   first_ray / hit / tof_hit [n_geom*n_tx][n_rx]   as rtus_match*   (hit, tof_hit nullable)
 *   tof, land_x [n_geom*n_tx][n_rays]     nullable: the per-ray arrays, stored only when asked for.  Without `tof` (what the
 *                                         reference's loop needs: main_rt.py:497-500 sums the segments of the HIT ray only) the
 *                                         four segment times are worked out only in waves that matched an element: 8 % less
 *                                         time at 8 M rays, the same tof_hit bits
 *   workspace  rtus_sweep_workspace_bytes(n_rays, n_geom, n_tx, n_rx) bytes, 64-byte aligned.
 *              RTUS_POLYLINE_READY here means: the previous call on this workspace was rtus_sweep_dev
 *              with the same alpha, n_rays, n_geom, n_tx and n_rx (the lens polyline is kept AND the
 *              matcher's scratch was left idle by that call).
 * ---------------------------------------------------------------------------------------- */
size_t rtus_sweep_workspace_bytes(int n_rays, int n_geom, int n_tx, int n_rx);

int rtus_sweep_dev(const rtus_lens *lens, const double *d_geoms, int n_geom,
                   const double *d_x_a, const double *d_z_a, int n_tx,
                   const double *d_alpha, const double *d_z_f, int n_rays,
                   const double *d_x_rx, int n_rx, double atol, double rtol,
                   int32_t *d_first_ray, uint8_t *d_hit, double *d_tof_hit,
                   double *d_tof, double *d_land_x,
                   void *d_workspace, size_t workspace_bytes, unsigned flags, void *stream);

int rtus_sweep(const rtus_lens *lens, const double *geoms, int n_geom,
               const double *x_a, const double *z_a, int n_tx,
               const double *alpha, const double *z_f, int n_rays,
               const double *x_rx, int n_rx, double atol, double rtol,
               int32_t *first_ray, uint8_t *hit, double *tof_hit,
               double *tof, double *land_x, unsigned flags, int device);

/* ------------------------------------------------------------------------------------------
 * Element x focal-point Fermat travel times through horizontal layers (BASELINE configs 2, 3, 5).
 * NOT IN THE REFERENCE (it has no planar interfaces) — the build's own solver, "parity
 * unpinned"; it replaces nothing in main_rt.py and is checked against oracle/ + closed forms.
 *
 *   z_if [n_if]    interface depths, strictly ascending (host memory, copied into kernel args)
 *   c    [n_if+1]  speeds; c[i] applies between interface i-1 and interface i
 *   xe,ze [n_e]    sources (elements), ze < z_if[0]
 *   xf,zf [n_f]    targets (focal points), zf > ze; the path stops in whichever layer holds zf
 *   tt   [n_e][n_f] travel times [s]; NaN where zf <= ze
 *   iters [n_e][n_f] uint8 nullable: Newton iterations used (diagnostic)
 *
 * rtus_tt_layers_batch_dev: n_batch independent problems of one shape and one medium in ONE launch — several
 * apertures and / or several target sets, the way the reference's driver sweeps 210 geometries (main_rt.py:464-467).
 * Problem b reads d_xe/d_ze + b*e_stride, d_xf/d_zf + b*f_stride and writes d_tt + b*t_stride (strides in doubles;
 * a stride of 0 shares that input between all problems; t_stride >= n_e*n_f).  A small problem (BASELINE config 2 is a
 * single round of 4 waves per SIMD) no longer pays a launch ramp and drain of its own.
 * ---------------------------------------------------------------------------------------- */
#define RTUS_MAX_LAYERS 8
/* Accuracy tier of the planar solver (flags of the *_ex entries, rtus_tt_layers_rows_dev, rtus_tt_layers_sorted_dev).  0: the travel time from an fp64
 * evaluation at the Newton iterate + its second-order Fermat expansion in an fp64 residual: <= 1e-13 relative (measured 3e-18 s
 * on BASELINE config 3).  RTUS_TT_TAUP_TAIL: from the tau-p form T = p X + sum (h_i/c_i) cos(theta_i), stationary in p, with the
 * second-order term from the fp32 residual (and, on a uniform pitch where the solution moves slowly from element to element, with
 * the term's coefficient carried over groups of four elements along the secant through the last two exactly formed values): at the
 * stopping threshold <= 6e-11 relative where the coefficient is formed, <= 1.3e-10 relative (~5e-15 s) where it is carried (8.4 % of
 * a second-order term of <= (tau/3)^2/8 T, tau = 3e-4, + 2e-11 of fp32 residual), ~3e-14 typically — five orders inside the
 * 1e-9 s bar of the north-star.  (Held to that bar on random, coarse and irregular apertures by scripts/fuzz_layers.py
 * --taup; round 3's version of this tier exceeded it — 2.8e-10 relative — on coarse random pitches.) */
#define RTUS_TT_TAUP_TAIL 0x1u

int rtus_tt_layers_dev(const double *z_if, const double *c, int n_if,
                       const double *d_xe, const double *d_ze, int n_e,
                       const double *d_xf, const double *d_zf, int n_f,
                       double *d_tt, uint8_t *d_iters, void *stream);

int rtus_tt_layers_batch_dev(const double *z_if, const double *c, int n_if,
                             const double *d_xe, const double *d_ze, int n_e, long long e_stride,
                             const double *d_xf, const double *d_zf, int n_f, long long f_stride,
                             double *d_tt, long long t_stride, int n_batch, void *stream);

int rtus_tt_layers(const double *z_if, const double *c, int n_if,
                   const double *xe, const double *ze, int n_e,
                   const double *xf, const double *zf, int n_f,
                   double *tt, uint8_t *iters, int device);

/* The same entries with the accuracy tier as an argument (flags: 0 or RTUS_TT_TAUP_TAIL; the un-suffixed entries above are
 * flags = 0).  iters is a diagnostic of the default tier's kernel: RTUS_ERR_INVALID_ARG with RTUS_TT_TAUP_TAIL.  bench.py's
 * headline times RTUS_TT_TAUP_TAIL; every caller — device pointers, host buffers, batches, several GPUs (below) — can ask for it. */
int rtus_tt_layers_ex_dev(const double *z_if, const double *c, int n_if,
                          const double *d_xe, const double *d_ze, int n_e,
                          const double *d_xf, const double *d_zf, int n_f,
                          double *d_tt, uint8_t *d_iters, unsigned flags, void *stream);
int rtus_tt_layers_batch_ex_dev(const double *z_if, const double *c, int n_if,
                                const double *d_xe, const double *d_ze, int n_e, long long e_stride,
                                const double *d_xf, const double *d_zf, int n_f, long long f_stride,
                                double *d_tt, long long t_stride, int n_batch, unsigned flags, void *stream);
int rtus_tt_layers_ex(const double *z_if, const double *c, int n_if,
                      const double *xe, const double *ze, int n_e,
                      const double *xf, const double *zf, int n_f,
                      double *tt, uint8_t *iters, unsigned flags, int device);

/* The aperture in ANY order.  The kernel starts each solve from the four previous elements of its workgroup's block, which pays
 * (1 evaluation instead of ~4.5) when consecutive elements are neighbours in space at one depth.  rtus_tt_layers_dev takes the
 * elements as they come; this entry sorts them on the device by (depth, position) first and stores each row where it belongs
 * (d_workspace: rtus_tt_layers_sort_workspace_bytes(n_e) bytes, 256-byte aligned; n_e <= 32768).  The result of an element does
 * not depend on the order the aperture was handed over in.  The host-buffer twin rtus_tt_layers does the same by itself (it sorts
 * on the host); flags: RTUS_TT_TAUP_TAIL or 0. */
size_t rtus_tt_layers_sort_workspace_bytes(int n_e);
int rtus_tt_layers_sorted_dev(const double *z_if, const double *c, int n_if,
                              const double *d_xe, const double *d_ze, int n_e,
                              const double *d_xf, const double *d_zf, int n_f,
                              double *d_tt, void *d_workspace, size_t workspace_bytes, unsigned flags, void *stream);

/* ------------------------------------------------------------------------------------------
 * Element x focal-point Fermat travel times through the reference's CURVED lens surface
 * (BASELINE config 4).  Interface = P(alpha) = h(alpha)(sin alpha, cos alpha) with h, dh/dalpha of
 * main_rt.py:180-214 (x_z_from_alpha :217-223, dz_dx_from_alpha :226-234); element in the lens
 * (c1), target in the water (c2).  The reference has no two-point solver (it only shoots rays from a
 * launch-angle grid, main_rt.py:479-482), so as a SOLVER this is the build's own; it is pinned to the
 * reference through Fermat <=> Snell: for a forward-traced ray, (A, F = pipe point) must give back
 * that ray's alpha and tof_1 + tof_2 (main_compare.py:514-515).
 *
 *   alpha_lo/hi    search interval for the refraction point's polar angle (e.g. -/+ alpha_max, main_rt.py:457)
 *   xe,ze [n_e]    elements;  xf,zf [n_f]  targets
 *   tt [n_e][n_f]  travel times;  alpha_out [n_e][n_f] nullable: polar angle of the refraction point
 * The entry is the LEAST time over [alpha_lo, alpha_hi] (Fermat).  The lens is aplanatic: around its focus T(alpha) is nearly flat
 * and has two local minima (an interior ray and an end of the interval, or both ends beyond the focus); the kernel follows one
 * minimum from element to element and looks at the whole interval wherever a second one can exist — a target pinned at an end, or
 * d2T/dalpha2 at the minimum below 0.125 h0 / c2 (7.5e-6 s/rad^2 for the reference lens: twice the largest value measured at an
 * interior minimum of a pair with two minima, scripts/study_lens_minima.py).  That threshold is CALIBRATED ON THE REFERENCE LENS
 * (main_rt.py:449-457) and scaled with the lens's own time h0 / c2; for another lens design check it with the same study.
 * ---------------------------------------------------------------------------------------- */
int rtus_tt_lens_dev(const rtus_lens *lens, double alpha_lo, double alpha_hi,
                     const double *d_xe, const double *d_ze, int n_e,
                     const double *d_xf, const double *d_zf, int n_f,
                     double *d_tt, double *d_alpha_out, void *stream);

int rtus_tt_lens(const rtus_lens *lens, double alpha_lo, double alpha_hi,
                 const double *xe, const double *ze, int n_e,
                 const double *xf, const double *zf, int n_f,
                 double *tt, double *alpha_out, int device);

int rtus_tt_lens_f32_dev(const rtus_lens *lens, double alpha_lo, double alpha_hi,
                         const float *d_xe, const float *d_ze, int n_e,
                         const float *d_xf, const float *d_zf, int n_f,
                         float *d_tt, float *d_alpha_out, void *stream);

int rtus_tt_lens_f32(const rtus_lens *lens, double alpha_lo, double alpha_hi,
                     const float *xe, const float *ze, int n_e,
                     const float *xf, const float *zf, int n_f,
                     float *tt, float *alpha_out, int device);

/* ------------------------------------------------------------------------------------------
 * Row shards of a travel-time table, and one call spread over several GPUs (SURVEY 8(b) "rtus_allgather(...)/multi-GPU
 * variant", 8(e)).  NOT IN THE REFERENCE (it has no device or process boundary at all).
 *
 * The table kernels solve `rows_per_block` consecutive elements per workgroup and start each solve from its predecessors
 * in the block.  rows_per_block is a function of the WHOLE table (rtus_table_rows_per_block), and the *_rows_dev entry
 * points keep workgroups aligned to the whole table's blocks: a shard [row0, row0 + n_rows) whose row0 is a multiple of
 * rows_per_block gets, bit for bit, the rows the one-launch table has (an unaligned shard is still correct to the solver's
 * accuracy; its first partial block has fewer predecessors).  rtus_shard_rows = rows per shard for n_shards equal shards,
 * rounded up to that multiple.
 *
 * rtus_*_multi: host buffers in, host table out, the rows spread over `devices[0 .. n_dev)` (a device may be listed more
 * than once: one arena and stream per entry); every device copies its block straight into the caller's rows — a host
 * result needs no exchange between the GPUs.
 * rtus_*_multi_dev: device i holds its own copies of the inputs (d_xe[i], d_ze[i]: ALL n_e elements; d_xf[i], d_zf[i]) and
 * of the padded table d_tt[i] [n_dev * rtus_shard_rows(...)][n_f]; it solves its row block in place on streams[i].
 * gather = 0 leaves the table sharded; gather = 1 reassembles it on every device by an in-place ncclAllGather over
 * single-process communicators (ncclCommInitAll; RCCL over xGMI, bound with dlopen at the first such call —
 * RTUS_ERR_UNSUPPORTED when librccl cannot be loaded or the communicators cannot be made).  Asynchronous.
 * ---------------------------------------------------------------------------------------- */
int rtus_table_rows_per_block(long long n_rows_total, int n_f, int elem_bytes);              /* elem_bytes: 8 (fp64) or 4 (fp32) */
long long rtus_shard_rows(long long n_rows_total, int n_f, int elem_bytes, int n_shards);

int rtus_tt_layers_rows_dev(const double *z_if, const double *c, int n_if,
                            const double *d_xe, const double *d_ze, int n_rows, long long row0, long long n_rows_total,
                            const double *d_xf, const double *d_zf, int n_f, double *d_tt, unsigned flags, void *stream);
int rtus_tt_lens_rows_dev(const rtus_lens *lens, double alpha_lo, double alpha_hi,
                          const double *d_xe, const double *d_ze, int n_rows, long long row0, long long n_rows_total,
                          const double *d_xf, const double *d_zf, int n_f, double *d_tt, double *d_alpha_out, void *stream);
int rtus_tt_lens_f32_rows_dev(const rtus_lens *lens, double alpha_lo, double alpha_hi,
                              const float *d_xe, const float *d_ze, int n_rows, long long row0, long long n_rows_total,
                              const float *d_xf, const float *d_zf, int n_f, float *d_tt, float *d_alpha_out, void *stream);

/* Diagnostic: the rows of rtus_tt_lens[_f32]_rows_dev (no alpha output) plus HOW they were solved, added to d_stats (device memory,
 * 5 x uint64, zeroed by the caller), counted in wave-elements (64 targets of one row): [0] T alone at the extrapolated start,
 * [1] one evaluation of T and dT/dalpha, [2] the safeguarded iteration, [3] of those: with a look at the whole search interval
 * (a target pinned at an end of it, or T nearly flat in alpha — around the lens focus two minima compete), [4] evaluations in [2]. */
int rtus_tt_lens_stats_dev(const rtus_lens *lens, double alpha_lo, double alpha_hi,
                           const double *d_xe, const double *d_ze, int n_rows, long long row0, long long n_rows_total,
                           const double *d_xf, const double *d_zf, int n_f, double *d_tt, unsigned long long *d_stats, void *stream);
int rtus_tt_lens_f32_stats_dev(const rtus_lens *lens, double alpha_lo, double alpha_hi,
                               const float *d_xe, const float *d_ze, int n_rows, long long row0, long long n_rows_total,
                               const float *d_xf, const float *d_zf, int n_f, float *d_tt, unsigned long long *d_stats, void *stream);

int rtus_tt_layers_multi(const double *z_if, const double *c, int n_if,
                         const double *xe, const double *ze, int n_e, const double *xf, const double *zf, int n_f,
                         double *tt, const int *devices, int n_dev);
int rtus_tt_lens_f32_multi(const rtus_lens *lens, double alpha_lo, double alpha_hi,
                           const float *xe, const float *ze, int n_e, const float *xf, const float *zf, int n_f,
                           float *tt, const int *devices, int n_dev);

/* ... with the accuracy tier (flags: 0 or RTUS_TT_TAUP_TAIL).  rtus_tt_layers_multi[_ex] sorts the aperture by (depth, position) on
 * the host first, as rtus_tt_layers does: the table is the one-device table bit for bit whatever order the elements come in. */
int rtus_tt_layers_multi_ex(const double *z_if, const double *c, int n_if,
                            const double *xe, const double *ze, int n_e, const double *xf, const double *zf, int n_f,
                            double *tt, const int *devices, int n_dev, unsigned flags);
int rtus_tt_layers_multi_ex_dev(const double *z_if, const double *c, int n_if,
                                const double *const *d_xe, const double *const *d_ze, int n_e,
                                const double *const *d_xf, const double *const *d_zf, int n_f, double *const *d_tt,
                                const int *devices, int n_dev, void *const *streams, int gather, unsigned flags);

int rtus_tt_layers_multi_dev(const double *z_if, const double *c, int n_if,
                             const double *const *d_xe, const double *const *d_ze, int n_e,
                             const double *const *d_xf, const double *const *d_zf, int n_f, double *const *d_tt,
                             const int *devices, int n_dev, void *const *streams, int gather);
int rtus_tt_lens_f32_multi_dev(const rtus_lens *lens, double alpha_lo, double alpha_hi,
                               const float *const *d_xe, const float *const *d_ze, int n_e,
                               const float *const *d_xf, const float *const *d_zf, int n_f, float *const *d_tt,
                               const int *devices, int n_dev, void *const *streams, int gather);

/* ------------------------------------------------------------------------------------------
 * Element x focal-point Fermat travel times through ONE curved interface given as a measured profile (immersion through a
 * pipe wall, a weld cap, a machined contour).  NOT IN THE REFERENCE — the build's own solver, "parity unpinned"; checked against
 * tests/surface_numpy.py (itself checked against mpmath at 40 digits) and, on a flat profile, against rtus_tt_layers.
 *
 *   x0, dx        the profile's grid: sample k at x_k = x0 + k dx, dx > 0
 *   zs   [n_s]    depths of the samples, n_s >= 4 (DEVICE memory in the _dev entry).  z points down.  The interface s(x) is the
 *                 NATURAL cubic spline through (x_k, zs[k]) on the extent [x0, x0 + (n_s - 1) dx]
 *   c1, c2        speed above the surface (medium 1, the couplant) and below it (medium 2, the part)
 *   xe,ze [n_e]   elements, in medium 1: an element that is not strictly above s over the whole extent (ze >= min s) gets a NaN
 *                 row.  Elements may lie horizontally outside the extent
 *   xf,zf [n_f]   focal points: x0 <= xf <= x0 + (n_s - 1) dx and zf > s(xf), else NaN.  There is no direct path through medium 1
 *   tt   [n_e][n_f]       travel times [s]: with S(x) = (x, s(x)) and, for x strictly inside the extent,
 *                         T(x) = |E - S(x)| / c1 + |S(x) - F| / c2,  the LEAST T OVER THE INTERIOR LOCAL MINIMA of T — the first
 *                         arriving ray that obeys Snell's law at the surface.  NaN when T has no interior local minimum (total
 *                         internal reflection, minima outside the extent).  Occlusion is NOT checked: on a wavy profile either leg
 *                         may cross the surface elsewhere.
 *   x_entry [n_e][n_f]    nullable: x of the winning entry point
 *
 * Guarantee: every interior local minimum whose basin spans at least one profile segment dx centred on it is found — the basin
 * running from the minimum to its neighbouring stationary points of T or to the ends of the extent; a minimum qualifies when
 * each neighbouring STATIONARY point is at least dx / 2 away (an end of the extent always does).  Narrower minima may be
 * missed; a missed minimum can only make the reported time later (or NaN), never earlier.  The entry is the least T over the
 * found minima where there are at most three of them.  With four or more, the three are chosen by a lower bound of each one's T
 * taken at a scan point next to it (spacing dx / 4: within T'' (dx / 4)^2 of the minimum's own T, ~2e-8 s on a 1 mm grid); the
 * least minimum can be left out where it is within that of the third chosen one, and the entry is then late by at most that much.
 * Determinism: an entry depends only on its element, its focal point, the profile and the speeds — not on which other elements
 * or focal points share the call (the bits of a row block or a focal-point subset are those of the whole table).
 *
 * The _dev entry runs a set-up kernel (the spline, into d_workspace: rtus_tt_surface_workspace_bytes(n_s) bytes, 256-byte
 * aligned) and the table kernel on `stream`: no allocation, no host synchronisation (capturable).  n_s <= 2^22, n_e <= 524280.
 * The host-buffer twin rtus_tt_surface stages everything through the device's arena.
 * ---------------------------------------------------------------------------------------- */
size_t rtus_tt_surface_workspace_bytes(int n_s);   /* 0 when n_s is out of range */
int rtus_tt_surface_dev(double x0, double dx, const double *d_zs, int n_s, double c1, double c2,
                        const double *d_xe, const double *d_ze, int n_e,
                        const double *d_xf, const double *d_zf, int n_f,
                        double *d_tt, double *d_x_entry, void *d_workspace, size_t workspace_bytes, void *stream);
int rtus_tt_surface(double x0, double dx, const double *zs, int n_s, double c1, double c2,
                    const double *xe, const double *ze, int n_e,
                    const double *xf, const double *zf, int n_f,
                    double *tt, double *x_entry, int device);

/* ------------------------------------------------------------------------------------------
 * Consumers of a travel-time table.  NOT IN THE REFERENCE, which stops at the travel times
 * (main_rt.py:497-504); checked against a NumPy restatement on synthetic point-scatterer data.
 *
 * rtus_focal_delays: transmit focal law, delays[e][f] = max over e' of tt[e'][f] - tt[e][f] — what element e must wait so
 *   that all wavefronts reach focal point f together.  NaN (no ray path) is ignored by the maximum and stays NaN.
 *   d_delays may be d_tt (in place).
 * rtus_tfm: total-focusing-method delay-and-sum over full-matrix-capture data,
 *   image[f] = sum over (tx, rx) of fmc[tx][rx][.] linearly interpolated at the sample position
 *   s = (tt_tx[tx][f] + tt_rx[rx][f] - t0) * fs, i.e. (1 - w) sample[i] + w sample[i + 1] with i = floor(s), w = s - i.  A
 *   position before the record (s < 0) or at / past its end (s >= n_t) contributes nothing; in [n_t - 1, n_t) the missing
 *   sample n_t counts as zero.  A pair without a ray path (NaN — or any non-finite or absurd travel time, |s| >= 1e8)
 *   contributes nothing.  (oracle/tfm_numpy.py is the same definition.)
 *     fmc     [n_tx][n_rx][n_t] float32 A-scans, fs samples per second, first sample at time t0
 *     tt_tx   [n_tx][n_f], tt_rx [n_rx][n_f]  travel times (rtus_tt_layers* / rtus_tt_lens outputs; may be one table)
 *     image   [n_f] float32
 * ---------------------------------------------------------------------------------------- */
int rtus_focal_delays_dev(const double *d_tt, int n_e, int n_f, double *d_delays, void *stream);
int rtus_focal_delays(const double *tt, int n_e, int n_f, double *delays, int device);

int rtus_tfm_dev(const float *d_fmc, int n_tx, int n_rx, int n_t, double fs, double t0,
                 const double *d_tt_tx, const double *d_tt_rx, int n_f, float *d_image, void *stream);
int rtus_tfm(const float *fmc, int n_tx, int n_rx, int n_t, double fs, double t0,
             const double *tt_tx, const double *tt_rx, int n_f, float *image, int device);

/* ------------------------------------------------------------------------------------------
 * Measuring the surface profile from the FMC itself ("adaptive TFM", immersion): image the couplant above the part with an
 * envelope TFM, take the depth of the surface echo in every column, then build tables through that profile (rtus_tt_surface) and
 * image the part (rtus_tfm).  NOT IN THE REFERENCE; checked against tests/autofocus_numpy.py.
 *
 * rtus_fmc_analytic: the analytic signal of every A-scan by an FIR Hilbert transformer,
 *   out[tx][rx][n] = (x[n], sum over m = -M..M of h[m] x[n - m]),   interleaved float32 complex [n_tx][n_rx][n_t][2],
 *   h[m] = 2 / (pi m) w[m] for odd m, 0 for even m (m = 0 included), w[m] = 0.54 + 0.46 cos(pi m / M) (the Hamming window over
 *   -M..M), n_taps = 2 M + 1 odd, 3 <= n_taps <= 255.  Samples outside the record count as zero.  The taps are formed in fp64 and
 *   rounded to fp32; the sum runs over m = 1, 3, .., M of h[m] (x[n - m] - x[n + m]) in fp32, in that order.  The output must not
 *   overlap the input (-1).  n_t <= 2^26.
 *
 * rtus_surface_find: the couplant envelope image and its column peak.
 *   a      [n_e][n_e][n_t][2]  a square analytic FMC (element e transmits and receives), as rtus_fmc_analytic makes it; fs, t0 as in
 *                              rtus_tfm
 *   xe,ze  [n_e]               elements (fp64; DEVICE memory in the _dev entry), c1 the couplant's speed
 *   columns x_k = x0 + k dx, k < n_s (rtus_tt_surface's grid); depths z_j = z_lo + j dz, j < n_z
 *   Pixel:  A[k][j] = | sum_tx sum_rx a[tx][rx](s) |,  s = (|E_tx - P| + |E_rx - P|) / c1 fs - t0 fs,  P = (x_k, z_j): straight
 *           rays, times formed in the kernel (each leg in fp64, rounded once to fp32 samples), no table.  Real and imaginary parts
 *           are interpolated linearly and separately, with rtus_tfm's edge rules: a position below 0 or at / past n_t contributes
 *           nothing, sample n_t counts as zero.  Accumulated in fp32 in a fixed order (tx, then rx ascending).
 *   Peak:   j* = the first index of the maximum of A[k][.].  z_peak[k] = NaN when j* is 0 or n_z - 1 (the surface is not inside
 *           the window) or when the maximum is 0 or not finite; otherwise z_lo + (j* + d) dz with the parabolic step
 *           d = (A- - A+) / (2 (A- - 2 A0 + A+)) over A[k][j* - 1 .. j* + 1] (fp64), clamped to [-1/2, 1/2].
 *   Outputs: z_peak [n_s] fp64; amp [n_s] float32 = A[k][j*] (NaN when the column holds a non-finite amplitude); image [n_s][n_z]
 *           float32, nullable.
 *   Determinism: a column's bits depend only on x_k and the other arguments, not on which other columns share the call.
 *   Limits: n_e <= 4096, 3 <= n_z <= 1024, n_s <= 2^24, 2 <= n_t <= 2^26 (-1 for invalid arguments, -5 past a limit, before any
 *   HIP call).  The _dev entry allocates nothing and does not synchronise (capturable).
 *   What the measurement assumes (the caller's part, not checked): an aperture without grating lobes (pitch below lambda / 2 in
 *   the couplant: with a coarser pitch a grating lobe can outshine the surface echo in a column), a depth window that holds the
 *   surface echo and no other strong echo, and moderate surface slopes (a steep facet sends its echo past the aperture: such columns
 *   come out dim and may be wrong).  Dim columns are unreliable; the Python layer (api.measure_surface) keeps only columns with
 *   amp >= threshold * max amp.
 * Measured on MI355X: 64 elements x 2048 samples, 256 columns x 256 depths: rtus_surface_find 300 us
 * (8.9e11 gathers/s, against rtus_tfm's 1.34e12 at 8 B per gather), rtus_fmc_analytic 26 us (63 taps).
 * ---------------------------------------------------------------------------------------- */
int rtus_fmc_analytic_dev(const float *d_fmc, int n_tx, int n_rx, int n_t, int n_taps, float *d_out, void *stream);
int rtus_fmc_analytic(const float *fmc, int n_tx, int n_rx, int n_t, int n_taps, float *out, int device);
int rtus_surface_find_dev(const float *d_a, int n_e, int n_t, double fs, double t0, const double *d_xe, const double *d_ze,
                          double c1, double x0, double dx, int n_s, double z_lo, double dz, int n_z,
                          double *d_z_peak, float *d_amp, float *d_image, void *stream);
int rtus_surface_find(const float *a, int n_e, int n_t, double fs, double t0, const double *xe, const double *ze,
                      double c1, double x0, double dx, int n_s, double z_lo, double dz, int n_z,
                      double *z_peak, float *amp, float *image, int device);

/* ------------------------------------------------------------------------------------------
 * rtus_tfm_analytic: the envelope TFM — rtus_tfm's delay-and-sum over an analytic (complex) FMC, through any travel-time table of
 * this library (rtus_tt_layers*, rtus_tt_lens*, rtus_tt_surface*) — and, optionally, the coherence factor.  NOT IN THE
 * REFERENCE; checked against tests/tfm_analytic_numpy.py.
 *   a       [n_tx][n_rx][n_t][2]  interleaved complex float32 (rtus_fmc_analytic's output, or any complex FMC); fs, t0,
 *                                 tt_tx [n_tx][n_f], tt_rx [n_rx][n_f] exactly as in rtus_tfm (the two tables may be one table)
 *   Sample position and edge rules: rtus_tfm's.  Each leg becomes (t fs - t0 fs / 2) in fp64, rounded once to fp32; a leg that is
 *           not finite or has |.| >= 1e8 samples has no path; the pair's position is s = tau_tx + tau_rx in fp32, i = floor(s),
 *           w = s - i; a position below 0 or at / past n_t contributes nothing, sample n_t counts as zero.  The real and imaginary
 *           parts are interpolated separately, each as fmaf(w, x[i + 1] - x[i], x[i]).
 *   image   [n_f][2]  S = (sum re, sum im) in fp32, accumulated in rtus_tfm's order (receive tiles of 64 elements, then tx
 *           ascending, then rx ascending inside the tile).  Consequence: image[f].re is bit-identical to rtus_tfm on the real
 *           parts of a, image[f].im to rtus_tfm on the imaginary parts.  The envelope is |S|.
 *   cf      [n_f] float32, nullable (null: nothing extra is computed).  The coherence factor (Mallart & Fink)
 *           cf = |S|^2 / (N E):  N = T R, T the number of tx with a path at f, R the number of rx with a path at f (a pair has a
 *           path iff both legs have one); E = the sum over the pairs of |interpolated complex sample|^2, fp32, in the same fixed
 *           order.  Formed in fp64 from the fp32 sums, clamped to [0, 1], rounded once to fp32.  cf = NaN when N = 0, 0 when
 *           E = 0 < N.  Pairs whose position falls outside the record count in N with value zero (so cf <= 1 by Cauchy-Schwarz).
 *           A CF-weighted envelope is |S| cf^p.
 *   Determinism: the bits of a focal point depend only on its own columns of the tables, not on n_f or on which other focal
 *           points share the call; passing cf does not change the bits of image.
 *   Limits: check_tfm's (image required, cf nullable) and 2 <= n_t <= 2^26 (16-byte samples addressed with 32-bit byte offsets):
 *           -1 for invalid arguments, -5 past a limit, before any HIP call.  The _dev entry allocates nothing and does not
 *           synchronise (capturable).  The host twin stages through the arena as rtus_tfm does (one table uploaded when
 *           tt_tx == tt_rx, cf downloaded only when asked for).
 * Measured on MI355X: 64 elements x 2048 samples, 256^2 focal points: 284 us, 281 us with cf (9.5e11 gathers/s,
 * 0.73x two rtus_tfm launches over split planes); 1024^2: 1.90 ms, 1.95 ms with cf (2.2e12 gathers/s).
 * ---------------------------------------------------------------------------------------- */
int rtus_tfm_analytic_dev(const float *d_a, int n_tx, int n_rx, int n_t, double fs, double t0,
                          const double *d_tt_tx, const double *d_tt_rx, int n_f,
                          float *d_image, float *d_cf, void *stream);
int rtus_tfm_analytic(const float *a, int n_tx, int n_rx, int n_t, double fs, double t0,
                      const double *tt_tx, const double *tt_rx, int n_f,
                      float *image, float *cf, int device);

/* ------------------------------------------------------------------------------------------
 * rtus_tfm_hmc, rtus_tfm_analytic_hmc: rtus_tfm and rtus_tfm_analytic over a HALF-MATRIX CAPTURE.  By reciprocity the A-scan of
 * (tx i, rx j) is that of (tx j, rx i), and most array controllers store only the records with i <= j.  NOT IN THE REFERENCE;
 * checked against tests/tfm_hmc_numpy.py.
 *   hmc     [n_pairs][n_t] float32 (analytic: [n_pairs][n_t][2]), n_pairs = n_e (n_e + 1) / 2.  The record of (i, j),
 *           0 <= i <= j < n_e, is number p(i, j) = i n_e - i (i - 1) / 2 + (j - i): the order of numpy.triu_indices(n_e); for a fixed
 *           i the records j = i .. n_e - 1 are contiguous.  fs, t0 as in rtus_tfm.
 *   tt_tx, tt_rx  [n_e][n_f] both: the same n_e elements transmit and receive.  The two may be one table (the same pointer).
 *   Sample position, interpolation, edge rules and the no-path rule: rtus_tfm's / rtus_tfm_analytic's (each leg's half of the
 *           position formed in fp64 and rounded once to fp32, the halves added in fp32).  With a_ij(s) the interpolated sample of
 *           record (i, j), s_ij built from tt_tx[i] and tt_rx[j], s_ji from tt_tx[j] and tt_rx[i]:
 *             S[f] = the sum of c_ij,   c_ii = a_ii(s_ii),   c_ij = a_ij(s_ij) + a_ij(s_ji) for i < j
 *           — the two of a pair added to each other FIRST, then to the running sum as one term.  In exact arithmetic this is rtus_tfm
 *           on the symmetric full matrix.  Order of the sum: blocks of 16 columns ascending; inside the block [c0, c0 + 16) first
 *           the rows i < c0 (i ascending, j ascending through the block), then the rows of the block (i ascending, j ascending
 *           from i).  Up to 16 elements this is: i ascending, j ascending from i.
 *   One table (tt_tx == tt_rx as pointers): s_ij == s_ji bit for bit and c_ij = 2 a_ij(s_ij) exactly, so the record is gathered
 *           ONCE and counted twice — 2080 gathers per focal point at 64 elements instead of 4096 — and the result has the bits of
 *           the two-table form called with two equal tables (samples whose double overflows fp32 apart).
 *   image   [n_f] float32 (analytic: [n_f][2], S = (sum re, sum im); each plane is rtus_tfm_hmc on that plane of the data, bit for
 *           bit)
 *   cf      [n_f] float32, nullable (analytic only): |S|^2 / (N E) with rtus_tfm_analytic's N = T R, formula, clamp and NaN rule;
 *           E = the sum, in the same order, of e_ii = |a_ii|^2, e_ij = |a_ij(s_ij)|^2 + |a_ij(s_ji)|^2 (pair first), each square
 *           formed as fmaf(im, im, re re).  Passing cf does not change the bits of image.
 *   Determinism: the bits of a focal point depend only on its own columns of the tables.
 *   Limits: 1 <= n_e <= 32768 (n_pairs fits an int; -1 otherwise) and rtus_tfm's / rtus_tfm_analytic's limits and codes for the
 *           rest.  The _dev entries allocate nothing and do not synchronise (capturable).  The host twins stage through the arena
 *           (one table uploaded when tt_tx == tt_rx).
 * Measured on MI355X (DESIGN.md §4 "Half-matrix capture", profiles/tfm_hmc_kernel.txt): 64 elements x 2048 samples, one table,
 * 256^2 focal points: 101 us real, 143 us analytic, 144 us with cf (0.54x / 0.53x / 0.53x rtus_tfm / rtus_tfm_analytic on the
 * unpacked block in the same run); 1024^2: 1.02 / 1.05 / 1.07 ms (0.54x / 0.55x / 0.55x).  Two tables: about the full-matrix time.
 * ---------------------------------------------------------------------------------------- */
int rtus_tfm_hmc_dev(const float *d_hmc, int n_e, int n_t, double fs, double t0,
                     const double *d_tt_tx, const double *d_tt_rx, int n_f, float *d_image, void *stream);
int rtus_tfm_hmc(const float *hmc, int n_e, int n_t, double fs, double t0,
                 const double *tt_tx, const double *tt_rx, int n_f, float *image, int device);
int rtus_tfm_analytic_hmc_dev(const float *d_a, int n_e, int n_t, double fs, double t0,
                              const double *d_tt_tx, const double *d_tt_rx, int n_f,
                              float *d_image, float *d_cf, void *stream);
int rtus_tfm_analytic_hmc(const float *a, int n_e, int n_t, double fs, double t0,
                          const double *tt_tx, const double *tt_rx, int n_f,
                          float *image, float *cf, int device);

/* ------------------------------------------------------------------------------------------
 * rtus_tfm_iq, rtus_tfm_iq_hmc: rtus_tfm_analytic and rtus_tfm_analytic_hmc with CARRIER-AWARE (IQ) interpolation.  The analytic
 * signal is an envelope times a carrier, and a straight line between two samples cuts the corner of the carrier's rotation: up
 * to 1 - cos(pi f0 / fs) per term (29 % at 4 samples per cycle), a different loss at every pixel.  Here the baseband signal is
 * interpolated and the carrier put back exactly, on the two samples the kernels load anyway.  NOT IN THE REFERENCE; checked
 * against tests/tfm_iq_numpy.py.
 *   f_demod [Hz], 0 <= f_demod < fs / 2: the carrier (demodulation) frequency.  nu = f_demod / fs in cycles per sample;
 *           R = (cos 2 pi nu, -sin 2 pi nu), formed on the host in fp64 and rounded to fp32; nu rounded to fp32.
 *   Every other argument: rtus_tfm_analytic's (rtus_tfm_analytic_hmc's).  Unchanged from there: the sample positions and their
 *           fp32 rounding; the edge rules (sample n_t reads as zero, a negative position contributes nothing, positions outside
 *           the record count in N with value zero); the no-path rule; the order of the sums (HMC: the pair first, one table: the
 *           record gathered once and counted twice); N = T R; cf's formula, clamp and NaN rule.
 *   The step, for a pair with a0, a1 the two loaded complex samples and w the fraction, all in fp32, every product and sum rounded
 *   by itself but the fmaf's:
 *             q = a1 R                     q.re = fmaf(a1.im, sin, a1.re cos),  q.im = fmaf(-a1.re, sin, a1.im cos)
 *             b = a0 + w (q - a0)          each part fmaf(w, q - a0, a0)
 *             p = b (cos 2 pi x, sin 2 pi x),  x = nu w in fp32
 *                                          p.re = fmaf(-b.im, sin, b.re cos),   p.im = fmaf(b.re, sin, b.im cos)
 *             S += p;  E += |p|^2;  cf = |S|^2 / (N E) as rtus_tfm_analytic
 *           with the phasor from the hardware's sine and cosine (argument in revolutions, x in [0, 0.5]).  For a(t) = e(t) exp(2 pi
 *           i f0 t) and f_demod = f0 this is the linear interpolation of the envelope e times the exact carrier.
 *   Consequences:
 *           f_demod = 0 gives rtus_tfm_analytic's (rtus_tfm_analytic_hmc's) image and cf BIT FOR BIT on finite data: R = (1, +0)
 *           and the phasor is (1, 0) exactly, and every product above is then exact.
 *           A position in [n_t - 1, n_t) gives (1 - w) a0 rotated by the phasor (the zero sample stays zero under R).
 *           Determinism: the bits of a focal point depend only on its own columns of the tables, not on n_f or on which other focal
 *           points share the call; passing cf does not change the bits of image.
 *   A wrong f_demod costs little: 10 % off costs 0.2 % of a TFM peak at 4 samples per cycle (DESIGN.md §4 "Carrier-aware
 *           interpolation"); the power-weighted mean frequency of the data is close enough.
 *   Limits: f_demod not finite, negative or >= fs / 2: -1; everything else rtus_tfm_analytic's (rtus_tfm_analytic_hmc's) codes;
 *           before any HIP call.  The _dev entries allocate nothing and do not synchronise (capturable).  The host twins stage
 *           through the arena as their twins do.
 * Measured on MI355X (DESIGN.md §4 "Carrier-aware interpolation", profiles/tfm_iq_kernel.txt; the linear twin in the same run = 1):
 * 64 elements x 2048 samples, 256^2 focal points: 272 us (1.02x), 280 us with cf (1.04x); half matrix, one table: 146 us (1.03x),
 * 155 us with cf (1.08x); two tables: 282 / 301 us (1.38x / 1.39x: VALU issue binds there).  Largest |image - oracle| / A: 2.3e-6.
 * ---------------------------------------------------------------------------------------- */
int rtus_tfm_iq_dev(const float *d_a, int n_tx, int n_rx, int n_t, double fs, double t0, double f_demod,
                    const double *d_tt_tx, const double *d_tt_rx, int n_f,
                    float *d_image, float *d_cf, void *stream);
int rtus_tfm_iq(const float *a, int n_tx, int n_rx, int n_t, double fs, double t0, double f_demod,
                const double *tt_tx, const double *tt_rx, int n_f,
                float *image, float *cf, int device);
int rtus_tfm_iq_hmc_dev(const float *d_a, int n_e, int n_t, double fs, double t0, double f_demod,
                        const double *d_tt_tx, const double *d_tt_rx, int n_f,
                        float *d_image, float *d_cf, void *stream);
int rtus_tfm_iq_hmc(const float *a, int n_e, int n_t, double fs, double t0, double f_demod,
                    const double *tt_tx, const double *tt_rx, int n_f,
                    float *image, float *cf, int device);

/* ------------------------------------------------------------------------------------------
 * rtus_tfm_frames, rtus_tfm_analytic_frames: TFM over a STACK of frames — an encoded scan along a pipe or a weld is hundreds to
 * thousands of captures of one shape, all imaged through the same travel-time tables on the same grid — in one call (a few
 * launches on the stream).  NOT IN THE REFERENCE; held bit for bit to the single-frame entries and to tests/das_exact_numpy.py.
 *   A stack is n_frames captures, frame-major: RF fmc [n_frames][n_tx][n_rx][n_t] float32; analytic a [n_frames][n_tx][n_rx][n_t][2].
 *   fs, t0, f_demod, tt_tx [n_tx][n_f], tt_rx [n_rx][n_f] (the two may be one table): as in rtus_tfm / rtus_tfm_analytic / rtus_tfm_iq,
 *           shared by every frame.
 *   images  [n_frames][n_f] float32 (RF) or [n_frames][n_f][2] (analytic); cf [n_frames][n_f] float32, nullable (analytic only).
 *   Frame k's output is, BIT FOR BIT, what the single-frame entry returns on frame k alone with the same tables, fs, t0 and
 *           f_demod: rtus_tfm (RF), rtus_tfm_analytic (f_demod == 0: the linear step itself, not rtus_tfm_iq's at a zero carrier),
 *           rtus_tfm_iq (f_demod > 0) — the same leg rule, edge rules, no-path rule and order of the sums.
 *   Determinism: the bits of a frame do not depend on n_frames, on its partner in a pair (below), on how a caller cuts the stack
 *           into calls, or on whether cf is asked for; the bits of a focal point depend only on its own columns of the tables.
 *   The PACKED layout of an RF stack: packed [n_pairs][n_tx][n_rx][n_t][2] float32, n_pairs = ceil(n_frames / 2); plane 0 of pair p
 *           is frame 2 p, plane 1 is frame 2 p + 1; plane 1 of the last pair of an odd stack is +0.0 everywhere.  rtus_tfm_analytic
 *           promises that S.re is rtus_tfm on the real parts and S.im rtus_tfm on the imaginary parts, so two RF frames stored
 *           sample-interleaved are imaged by ONE 16-byte gather per (pair of elements, focal point) where two launches of rtus_tfm
 *           issue two 8-byte ones — and the vector-memory address path, not the bytes, paces the gather.
 *   rtus_fmc_pack_frames_floats: the floats of the packed stack, 2 n_pairs n_tx n_rx n_t; 0 when a size is not positive or the
 *           count does not fit 2^62 bytes.
 *   rtus_fmc_pack_frames_dev: frame-major stack -> packed (writes the zero plane of an odd stack).  n_t >= 1.  d_packed must be
 *           8-byte aligned and must not overlap d_fmc (-1).  A streaming copy: 4 n_frames n_tx n_rx n_t bytes read, 8 n_pairs ...
 *           written.  A streaming caller may pack each arriving pair by itself (n_frames = 2 at the pair's place), or have its
 *           acquisition write the layout directly.
 *   rtus_tfm_frames_dev takes the PACKED stack (n_frames says whether the last pair has one frame: its images row 2 p + 1 does not
 *           exist and is not written).  The host twin rtus_tfm_frames takes the FRAME-MAJOR stack, uploads it as it is and packs on
 *           the device in the arena.
 *   Limits: a null pointer (cf apart), a non-positive size, n_t < 2, fs not positive and finite, t0 not finite, f_demod outside
 *           [0, fs / 2): -1.  n_t > 2^26 (rtus_tfm_analytic's limit: 16-byte positions, 32-bit byte offsets), or more than
 *           2^31 - 1 workgroups — n_pairs ceil(n_f / 256) for RF, n_frames ceil(n_f / 256) for analytic: -5.  All before any HIP
 *           call.  The _dev entries allocate nothing and do not synchronise (capturable).
 * Kernels, the workgroup order and the figures: DESIGN.md §4 "TFM over a stack of frames" (profiles/tfm_frames_kernel.txt).
 *           A call is one launch per about 2304 workgroups (nine images of 256^2 focal points, one of 1024^2): a launch that grows with
 *           the stack was measured 1.2x to 1.7x slower at 32 frames.
 * Measured on MI355X, 64 elements x 2048 samples, one table, medians of 50 alternating repetitions, time per frame; the estimate
 * was 0.73x to 0.5x of a loop over rtus_tfm_dev:
 *   256^2 focal points:  loop of rtus_tfm_dev 226 us; pack + rtus_tfm_frames_dev 146 us at 8 frames (0.65x), 162 us at 9 (0.72x: the
 *           fifth pair is half empty), 157 us at 32 (0.69x); on an already packed stack 135 / 149 / 142 us (0.60x / 0.66x / 0.63x);
 *           the pack alone 12 us per frame.
 *   1024^2: loop 1.92 ms; pack + stack 1.00 ms at 8 frames (0.52x), 1.11 ms at 9 (0.58x), 0.98 ms at 32 (0.51x); packed 0.97 /
 *           1.08 / 0.97 ms (0.51x / 0.56x / 0.50x).
 *   rtus_tfm_analytic_frames_dev against a loop of rtus_tfm_analytic_dev: 0.97x / 0.95x / 0.99x at 256^2 (280 against 289 us per
 *           frame at 8 frames), 1.00x at 1024^2 (1.94 ms): the same gathers; what it saves is the calls.
 * ---------------------------------------------------------------------------------------- */
size_t rtus_fmc_pack_frames_floats(int n_frames, int n_tx, int n_rx, int n_t);
int rtus_fmc_pack_frames_dev(const float *d_fmc, int n_frames, int n_tx, int n_rx, int n_t, float *d_packed, void *stream);
int rtus_tfm_frames_dev(const float *d_packed, int n_frames, int n_tx, int n_rx, int n_t, double fs, double t0,
                        const double *d_tt_tx, const double *d_tt_rx, int n_f, float *d_images, void *stream);
int rtus_tfm_frames(const float *fmc, int n_frames, int n_tx, int n_rx, int n_t, double fs, double t0,
                    const double *tt_tx, const double *tt_rx, int n_f, float *images, int device);
int rtus_tfm_analytic_frames_dev(const float *d_a, int n_frames, int n_tx, int n_rx, int n_t, double fs, double t0, double f_demod,
                                 const double *d_tt_tx, const double *d_tt_rx, int n_f,
                                 float *d_images, float *d_cf, void *stream);
int rtus_tfm_analytic_frames(const float *a, int n_frames, int n_tx, int n_rx, int n_t, double fs, double t0, double f_demod,
                             const double *tt_tx, const double *tt_rx, int n_f,
                             float *images, float *cf, int device);

/* ------------------------------------------------------------------------------------------
 * rtus_tfm_frames_i16: rtus_tfm_frames over a stack of INT16 frames — the samples as an array controller delivers them — with
 * four frames per 16-byte gather, half the bytes uploaded and half the device memory of the float32 route.  NOT IN THE REFERENCE;
 * held bit for bit to rtus_tfm on the frames converted to float32 and to tests/das_exact_numpy.py.
 *   A stack is n_frames captures, frame-major: fmc [n_frames][n_tx][n_rx][n_t] int16.  fs, t0, tt_tx, tt_rx, images [n_frames][n_f]
 *           float32: as in rtus_tfm_frames.
 *   Frame k's image is, BIT FOR BIT, rtus_tfm on frame k converted to float32 (the conversion is exact): the same leg rule, edge
 *           rules, no-path rule and order of the sums.  There is no gain argument: the image is linear in the data, so a caller
 *           scales the image.  Determinism: as rtus_tfm_frames — no bit depends on n_frames, on the other frames of a quad, or on
 *           how a caller cuts the stack into calls.
 *   The PACKED layout: packed [n_quads][n_tx][n_rx][n_t][4] int16, n_quads = ceil(n_frames / 4); plane c of quad q is frame 4 q + c;
 *           the planes of the absent frames of the last quad are 0.  A sample position is 8 bytes — the record shape of a pair of
 *           float32 frames — so ONE 16-byte gather brings two neighbouring samples of FOUR frames.
 *   rtus_fmc_pack_frames_i16_words: the int16 values of the packed stack, 4 n_quads n_tx n_rx n_t; 0 when a size is not positive
 *           or the count does not fit 2^62 bytes.
 *   rtus_fmc_pack_frames_i16_dev: frame-major stack -> packed (writes the zero planes of a ragged last quad).  n_t >= 1.  d_packed
 *           must be 8-byte aligned, d_fmc 2-byte aligned, and the two must not overlap (-1).  A streaming interleave: 2 n_frames
 *           n_tx n_rx n_t bytes read, 8 n_quads ... written; 16-byte loads and stores when a frame is a multiple of 8 samples and
 *           both pointers are 16-byte aligned, 2-byte loads and 8-byte stores otherwise.
 *   rtus_tfm_frames_i16_dev takes the PACKED stack (n_frames says how many frames the last quad holds: the images rows of its
 *           absent frames do not exist and are not written).  The host twin rtus_tfm_frames_i16 takes the FRAME-MAJOR int16 stack,
 *           uploads it as int16 and packs on the device in the arena.
 *   Limits: rtus_tfm_frames' — a null pointer, a non-positive size, n_t < 2, fs not positive and finite, t0 not finite: -1.
 *           n_t > 2^26, or more than 2^31 - 1 workgroups, n_quads ceil(n_f / 256): -5.  All before any HIP call.  The _dev entries
 *           allocate nothing and do not synchronise (capturable).
 * Kernels and the figures: DESIGN.md §4 "TFM over int16 frame stacks" (profiles/tfm_frames_i16_kernel.txt).
 *           A call is one launch per about 2304 workgroups, counted in quads (rtus_tfm_frames' rule; measured again for quads: the
 *           whole stack in one launch was equal at 256^2 and 1 % to 2.5 % faster at 1024^2, one quad per launch 2 % to 6 % slower at 256^2).
 * Measured on MI355X, 64 elements x 2048 samples, one table, medians of 50 alternating repetitions, time per frame, against
 * rtus_tfm_frames_dev on a float32-packed stack in the same run (= 1); the estimate before the measurement was 0.55x to 0.7x:
 *   256^2 focal points:  packed float32 133 / 149 / 138 us at 8 / 9 / 32 frames; rtus_tfm_frames_i16_dev on a packed int16 stack
 *           71 / 91 / 74 us (0.53x / 0.61x / 0.54x; 9 frames are three quads, the third a quarter full); int16 pack + stack 78 / 101 /
 *           101 us (0.54x / 0.62x / 0.66x of float32 pack + stack); the int16 pack alone 7 to 10 us per frame (float32: 12).
 *   1024^2: packed float32 0.97 / 1.08 / 0.98 ms; packed int16 0.72 / 0.97 / 0.72 ms (0.74x / 0.89x / 0.74x: outside the estimate — a
 *           quad's launch takes 1.48x a pair's there, the decode is not hidden behind the gathers); int16 pack + stack 0.73 / 0.97 /
 *           0.73 ms (0.74x / 0.88x / 0.74x of float32 pack + stack).
 *   The host twins on 8 frames from pageable memory (268 MB as float32, 134 MB as int16), wall time: 6.6 ms against 3.7 ms at 256^2
 *           (0.56x), 24.0 ms against 19.5 ms at 1024^2 (0.81x).
 * ---------------------------------------------------------------------------------------- */
size_t rtus_fmc_pack_frames_i16_words(int n_frames, int n_tx, int n_rx, int n_t);
int rtus_fmc_pack_frames_i16_dev(const short *d_fmc, int n_frames, int n_tx, int n_rx, int n_t, short *d_packed, void *stream);
int rtus_tfm_frames_i16_dev(const short *d_packed, int n_frames, int n_tx, int n_rx, int n_t, double fs, double t0,
                            const double *d_tt_tx, const double *d_tt_rx, int n_f, float *d_images, void *stream);
int rtus_tfm_frames_i16(const short *fmc, int n_frames, int n_tx, int n_rx, int n_t, double fs, double t0,
                        const double *tt_tx, const double *tt_rx, int n_f, float *images, int device);

/* ------------------------------------------------------------------------------------------
 * rtus_tfm_frames_hmc_i16, rtus_tfm_frames_hmc: rtus_tfm_hmc over a STACK of half-matrix frames — what a recorded scan is: int16
 * (or float32) samples, the n_pairs = n_e (n_e + 1) / 2 records with tx <= rx, hundreds of captures through the same tables —
 * four int16 frames (two float32 frames) per 16-byte gather and one gather per record.  NOT IN THE REFERENCE; held bit for bit to
 * rtus_tfm_hmc on each frame and to tests/das_exact_numpy.py.
 *   A stack is n_frames captures, frame-major: hmc [n_frames][n_pairs][n_t], int16 or float32, the records in rtus_tfm_hmc's
 *           order.  n_e, fs, t0, tt_tx, tt_rx [n_e][n_f]: as in rtus_tfm_hmc; images [n_frames][n_f] float32.
 *   The contract.  Frame k's image is, BIT FOR BIT, rtus_tfm_hmc on frame k converted to float32 (exact): its pair rule, weights,
 *           edge rules, no-path rule and order of summation.  No bit depends on n_frames, on the other planes of a quad or pair, or
 *           on how the stack is cut into calls or launches.  tt_tx == tt_rx AS POINTERS selects the one-table kernels (one gather
 *           per record, weight 2 off the diagonal), whose images have the bits of the two-table call with equal tables, as
 *           rtus_tfm_hmc promises.
 *   The PACKED layouts are rtus_tfm_frames[_i16]'s with one "transmit row" of n_pairs records: packed [n_quads][n_pairs][n_t][4]
 *           int16 (plane c of quad q is frame 4 q + c) and packed [n_fpairs][n_pairs][n_t][2] float32 (plane c of pair p is frame
 *           2 p + c); the planes of absent frames are 0.  rtus_fmc_pack_frames[_i16]_dev make them with (n_tx, n_rx) = (1, n_pairs).
 *           A sample position is 8 bytes either way — the record shape of analytic HMC data.
 *   The _dev entries take the PACKED stack (n_frames says how many frames the last quad or pair holds: the images rows of its absent
 *           frames do not exist and are not written), allocate nothing and do not synchronise (capturable).  The host twins take
 *           the FRAME-MAJOR stack, upload it in its own type and pack on the device in the arena.
 *   Limits: a null pointer, a non-positive size, n_e > 32768, n_t < 2, fs not positive and finite, t0 not finite: -1.  n_t > 2^26,
 *           or more than 2^31 - 1 workgroups (n_quads or n_fpairs times ceil(n_f / 256)): -5.  All before any HIP call.
 *   Memory: the int16 route uploads and holds half the bytes of a float32 HMC stack and about half (n_e + 1) / (2 n_e) of an int16
 *           full-matrix stack, by construction.
 * Kernels, resources and the figures: DESIGN.md §4 "TFM over half-matrix frame stacks" (profiles/tfm_frames_hmc_kernel.txt).  A
 *           call is one launch per about 2304 workgroups, counted in quads or pairs (rtus_tfm_frames' rule, not measured again).
 * Measured on MI355X, 64 elements (2080 records) x 2048 samples, medians of 50 alternating repetitions, two separate runs (they differ
 * by at most 0.012 in a ratio), time per frame with the pack included, against (a) a loop of rtus_tfm_hmc_dev on the float32 frames
 * and (b) rtus_tfm_frames_i16_dev on the stack expanded to full matrices and already packed, in the same run.  The estimate before
 * the measurement, from the ratios above: 0.35x to 0.45x of (a) at 256^2.
 *   one table, 256^2 focal points, 8 / 9 / 32 frames: (a) 116 / 120 / 123 us, (b) 72 / 100 / 83 us, rtus_tfm_frames_hmc_i16_dev with its
 *           pack 42 / 53 / 39 us: 0.36x / 0.44x / 0.32x of (a), 0.58x / 0.53x / 0.47x of (b); already packed 37 / 48 / 35 us.
 *   one table, 1024^2: (a) 1.03 / 1.03 / 1.03 ms, (b) 0.74 / 0.98 / 0.73 ms, int16 HMC stack 0.39 / 0.52 / 0.39 ms: 0.38x / 0.51x / 0.38x of
 *           (a), 0.53x / 0.54x / 0.53x of (b).  The bar — faster than both with one table and whole quads, by more than the runs
 *           differ — is met at both sizes.
 *   two tables (reported): 256^2 61 / 80 / 59 us against (a) 223 / 227 / 231 and (b) 74 / 102 / 109; 1024^2 0.78 / 1.04 / 0.78 ms against
 *           (a) 2.10 / 2.09 / 2.10 and (b) 0.80 / 1.06 / 0.79: two gathers per record, so level with the full matrix there (0.96x to 0.99x).
 *   float32 pairs with their pack, one table: 75 / 82 / 74 us at 256^2 (0.60x to 0.68x of (a)), 0.53 / 0.59 / 0.53 ms at 1024^2 (0.51x to 0.57x).
 *   The host twins on 8 frames from pageable memory, wall time: 2.3 ms (68 MB up) against 8.6 ms for a loop of rtus_tfm_hmc on float32
 *           frames (136 MB up, and the tables with every call) and 3.7 ms for rtus_tfm_frames_i16 on the expanded stack (134 MB up) at
 *           256^2; 15.1 ms against 88.6 ms and 19.5 ms at 1024^2.
 * ---------------------------------------------------------------------------------------- */
int rtus_tfm_frames_hmc_i16_dev(const short *d_packed, int n_frames, int n_e, int n_t, double fs, double t0,
                                const double *d_tt_tx, const double *d_tt_rx, int n_f, float *d_images, void *stream);
int rtus_tfm_frames_hmc_i16(const short *hmc, int n_frames, int n_e, int n_t, double fs, double t0,
                            const double *tt_tx, const double *tt_rx, int n_f, float *images, int device);
int rtus_tfm_frames_hmc_dev(const float *d_packed, int n_frames, int n_e, int n_t, double fs, double t0,
                            const double *d_tt_tx, const double *d_tt_rx, int n_f, float *d_images, void *stream);
int rtus_tfm_frames_hmc(const float *hmc, int n_frames, int n_e, int n_t, double fs, double t0,
                        const double *tt_tx, const double *tt_rx, int n_f, float *images, int device);

/* ------------------------------------------------------------------------------------------
 * rtus_tfm_envelope_frames_hmc[_i16]: ENVELOPE TFM over a stack of half-matrix frames, the analytic signal formed on the device —
 * raw int16 (or float32) samples up, complex or magnitude images down, nothing in between touches the host.  NOT IN THE REFERENCE;
 * held bit for bit to the frame-by-frame route through rtus_fmc_analytic and rtus_tfm_analytic_hmc / rtus_tfm_iq_hmc.
 *   A stack: hmc [n_frames][n_pairs][n_t], int16 or float32, frame-major, the records in rtus_tfm_hmc's order.  n_taps: the Hilbert
 *           transformer's (rtus_fmc_analytic), odd in [3, 255].  fs, t0, tt_tx, tt_rx [n_e][n_f]: as in rtus_tfm_hmc.  f_demod in
 *           [0, fs / 2): 0 interpolates linearly, > 0 is rtus_tfm_iq's carrier-aware step.  flags: 0 or RTUS_ENV_MAGNITUDE.
 *           images [n_frames][n_f][2] float32 (8-byte aligned), or [n_frames][n_f] with RTUS_ENV_MAGNITUDE; cf [n_frames][n_f] or null.
 *   The contract.  Frame k's complex image is, BIT FOR BIT, what rtus_tfm_analytic_hmc returns on rtus_fmc_analytic of frame k
 *           converted to float32 (exact), called with (n_tx, n_rx) = (1, n_pairs) and the same n_taps; with f_demod > 0 it is
 *           rtus_tfm_iq_hmc's image; cf is the coherence factor of that same call.  No bit depends on n_frames, on a frame's partners
 *           in a quad or pair, on how the stack is cut into calls or launches, on whether cf is asked for, or on which internal
 *           route ran.  tt_tx == tt_rx AS POINTERS selects the one-table kernels, as in rtus_tfm_frames_hmc.
 *   RTUS_ENV_MAGNITUDE: m = (float) sqrt((double) re * re + (double) im * im) of the complex image — the products exact in fp64,
 *           one rounding in the sum, a correctly rounded fp64 sqrt, one rounding to float; in NumPy
 *           np.sqrt(re.astype(f8)**2 + im.astype(f8)**2).astype(f4).  Half the download; no intermediate overflows.
 *   Routes.  int16 frames with f_demod == 0 and cf null take the SPLIT-PLANE route: rtus_tfm_analytic_hmc's image is, plane by plane,
 *           rtus_tfm_hmc of that plane; the real plane of an analytic int16 frame is the frame, so the real parts of four frames come
 *           from one gather per record (rtus_tfm_frames_hmc_i16's kernel on the raw quads) and the imaginary parts from the float32
 *           pair kernel on the Hilbert planes, which the transformer writes pair-packed: three 16-byte gathers per record and four
 *           frames where the complex kernel issues four; a streaming kernel joins the planes.  Every other case takes the COMPLEX
 *           route: frame by frame, the transformer into one frame's block of the workspace, then rtus_tfm_analytic_hmc's /
 *           rtus_tfm_iq_hmc's kernel on that block: two launches per frame, the parent's kernels for the image.
 *   rtus_fmc_analytic_i16[_dev]: rtus_fmc_analytic on int16 samples: out has its bits on the samples as float32 (d_out 8-byte aligned).
 *   rtus_fmc_hilbert_pairs_i16_dev: the Hilbert planes alone of a frame-major int16 stack [n_frames][n_scans][n_t], in the float32
 *           pair-packed layout d_packed [n_fpairs][n_scans][n_t][2] that rtus_tfm_frames_hmc_dev reads: plane c of pair p is the
 *           imaginary part of rtus_fmc_analytic of frame 2 p + c; the absent frame of an odd stack is +0.0.  d_packed 8-byte aligned,
 *           not overlapping d_fmc (-1); more than 2^31 - 1 workgroups, n_fpairs n_scans ceil(n_t / 1024): -5.
 *   rtus_tfm_envelope_frames_hmc_workspace_bytes: the bytes the _dev entries need for these sizes (i16: 1 for the int16 entry;
 *           want_cf: 1 when cf is not null); 0 for a size that is not positive, n_e > 32768, an unknown flag, f_demod negative or
 *           not finite, or a sum past 2^62.  The _dev entries take the FRAME-MAJOR stack and pack inside d_work (64-byte aligned),
 *           allocate nothing and do not synchronise (capturable).  The host twins upload the stack in its own type and work in the arena.
 *   Limits: rtus_tfm_frames_hmc's (-1: a null pointer, a non-positive size, n_e > 32768, n_t < 2, fs not positive and finite, t0 not
 *           finite; -5: n_t > 2^26, or more than 2^31 - 1 workgroups), and: n_taps not odd in [3, 255], f_demod outside [0, fs / 2),
 *           an unknown flag, a misaligned pointer: -1; more than 2^31 - 1 A-scan tiles, n_frames n_pairs ceil(n_t / 1024): -5; a
 *           workspace that is null, not 64-byte aligned or too small: -4.  All before any HIP call.
 * Kernels, resources and the figures: DESIGN.md §4 "Envelope TFM over half-matrix frame stacks" (profiles/
 *           tfm_envelope_frames_hmc_kernel.txt).
 * Measured on MI355X, 2026-10-21, 64 elements (2080 records) x 2048 int16 samples, medians of 50 alternating repetitions, two separate
 * runs (with one table they differ by at most 0.002 in a ratio, with two by 0.034; run 1 quoted), time per frame, against (L) a device loop per frame of
 * rtus_fmc_analytic_dev and rtus_tfm_analytic_hmc_dev on float32 frames in the same run.  ESTIMATED before the measurement, composed
 * from figures of separate runs: the split-plane route about 0.8x of (L) at 256^2 focal points and 0.9x at 1024^2, the complex route
 * about 1.0x.
 *   one table, 256^2, 8 / 9 / 32 frames: (L) 162 / 162 / 161 us; the int16 _dev entry on its split-plane route, pack, Hilbert and
 *           combine included, 119 / 140 / 118 us (0.74x / 0.86x / 0.73x), the same with the magnitude output; with cf (the complex
 *           route) 162 / 162 / 163 us (1.00x / 1.00x / 1.01x).
 *   one table, 1024^2: (L) 1.05 / 1.05 / 1.05 ms; split-plane 0.93 / 1.11 / 0.93 ms (0.89x / 1.06x / 0.88x: nine frames are
 *           three quads and five pairs with the last ones a quarter and half full — slower than the loop there); complex route
 *           1.08 / 1.09 / 1.08 ms (1.03x / 1.04x / 1.03x).
 *   two tables (reported, 8 and 32 frames): split-plane 0.67 to 0.69x at 256^2, 0.85 to 0.87x at 1024^2; complex route 1.05x, 1.01 to 1.02x.
 *   The host twin on 8 frames from pageable memory against the Python loop route (widen, rtus_fmc_analytic, rtus_tfm_analytic_hmc per
 *           frame), wall time, which depends on the host's pageable copies: 3.07 ms (102 MB up, 4 MB down) against 46.51 ms
 *           (677 MB up, 277 MB down) at 256^2, 20.92 ms against 126.02 ms at 1024^2; with the magnitude output 2.97 and 20.27 ms.
 * ---------------------------------------------------------------------------------------- */
#define RTUS_ENV_MAGNITUDE 1
int rtus_fmc_analytic_i16_dev(const short *d_fmc, int n_tx, int n_rx, int n_t, int n_taps, float *d_out, void *stream);
int rtus_fmc_analytic_i16(const short *fmc, int n_tx, int n_rx, int n_t, int n_taps, float *out, int device);
int rtus_fmc_hilbert_pairs_i16_dev(const short *d_fmc, int n_frames, int n_scans, int n_t, int n_taps, float *d_packed, void *stream);
size_t rtus_tfm_envelope_frames_hmc_workspace_bytes(int n_frames, int n_e, int n_t, int n_f, int i16, double f_demod, int want_cf,
                                                    int flags);
int rtus_tfm_envelope_frames_hmc_i16_dev(const short *d_hmc, int n_frames, int n_e, int n_t, int n_taps, double fs, double t0,
                                         double f_demod, const double *d_tt_tx, const double *d_tt_rx, int n_f, int flags,
                                         float *d_images, float *d_cf, void *d_work, size_t work_bytes, void *stream);
int rtus_tfm_envelope_frames_hmc_i16(const short *hmc, int n_frames, int n_e, int n_t, int n_taps, double fs, double t0,
                                     double f_demod, const double *tt_tx, const double *tt_rx, int n_f, int flags,
                                     float *images, float *cf, int device);
int rtus_tfm_envelope_frames_hmc_dev(const float *d_hmc, int n_frames, int n_e, int n_t, int n_taps, double fs, double t0,
                                     double f_demod, const double *d_tt_tx, const double *d_tt_rx, int n_f, int flags,
                                     float *d_images, float *d_cf, void *d_work, size_t work_bytes, void *stream);
int rtus_tfm_envelope_frames_hmc(const float *hmc, int n_frames, int n_e, int n_t, int n_taps, double fs, double t0,
                                 double f_demod, const double *tt_tx, const double *tt_rx, int n_f, int flags,
                                 float *images, float *cf, int device);

/* ------------------------------------------------------------------------------------------
 * Plane-wave imaging (PWI): a few dozen plane waves, each fired by the whole aperture with a linear delay law and received on every
 * element.  The transmit leg is a table with one row per angle, tt_pw [n_a][n_f]; the receive leg is an element table (rtus_tt_*)
 * and the delay-and-sum is rtus_tfm / rtus_tfm_analytic with tt_tx = tt_pw.  NOT IN THE REFERENCE; checked against
 * tests/pwi_numpy.py (itself checked against mpmath at 40 digits and a brute-force Huygens minimum).
 *
 * Array and angle.  The array is linear and horizontal at depth z_a, spanning [x_lo, x_hi], in medium 1 (speed c1; c[0] for
 * layers).  A plane wave has angle t, measured in medium 1 from +z towards +x, with |t| < pi/2.  Let u = (sin t, cos t) and
 * x_ref = x_lo if sin t >= 0, else x_hi.  Element e fires at d_e(t) = (x_e - x_ref) sin t / c1 >= 0, so time zero is the first
 * firing.  These are the delays the user loads into the instrument (the Python layer's pw_delays returns them).
 *
 * rtus_pw_layers: planar layers (z_if, c as in rtus_tt_layers, HOST memory; z_a < z_if[0]).  With p = sin t / c[0] and h_i the
 *   vertical extent of layer i between z_a and zf:
 *       t(F) = (xf - x_ref) p + sum_i h_i sqrt(1/c_i^2 - p^2)
 *   The entry is NaN when any of these holds: zf <= z_a; p c_i >= 1 in a layer the path crosses (evanescent); t is not finite or
 *   |t| >= pi/2; F is not insonified.  F is insonified when the ray traced back from F meets the array line inside the aperture:
 *   x_back = xf - sum_i h_i p c_i / sqrt(1 - p^2 c_i^2) must lie in [x_lo, x_hi] (inclusive).  A focal point on an interface
 *   depth belongs to the layer above it.  The square roots are formed once per (angle, layer) in the kernel.
 *
 * rtus_pw_surface: a measured surface (the spline, grid, extent and focal-point rules of rtus_tt_surface; c1 above, c2 below).
 *   With S(x) = (x, s(x)):
 *       T(x) = ((x - x_ref) sin t + (s(x) - z_a) cos t) / c1 + |S(x) - F| / c2
 *   An entry x is insonified when x - (s(x) - z_a) tan t lies in [x_lo, x_hi].  The table entry is the least T over the interior
 *   local minima of T at insonified entries.  It is NaN when there is none, when the profile is not strictly below z_a (z_a >=
 *   min s: the whole table is NaN), for an angle that is not finite or has |t| >= pi/2, and under rtus_tt_surface's focal-point
 *   rules.  x_entry [n_a][n_f] is optional, as in rtus_tt_surface.
 *   Guarantee: rtus_tt_surface's, with the band edges counting like stationary points: a minimum is found when its neighbouring
 *   stationary points and band edges are at least dx / 2 away.
 *   Determinism: an entry's bits depend only on its angle, its focal point, the profile, the array and the speeds; subsets or
 *   reorderings of angles or focal points give the same bits.
 *   d_workspace: rtus_tt_surface_workspace_bytes(n_s) bytes, 256-byte aligned (-4 otherwise).
 *
 * rtus_fmc_synth_tx: synthesis of any transmit delay law from an FMC,
 *       out[v][rx][n] = sum over tx ascending of x_{tx,rx}(n - d[v][tx] fs)
 *   fmc [n_tx][n_rx][n_t] float32 (fs samples per second), delays [n_v][n_tx] in seconds (DEVICE memory in the _dev entry): plane
 *   waves, diverging waves and sub-apertures all fit.  x is the record, linearly interpolated; indices outside [0, n_t) count as
 *   zero.  For each (v, tx) the shift s = d fs is formed once in fp64: m = ceil(s), the position n - s lies between samples
 *   i = n - m and i + 1 with weight w = m - s, rounded once to fp32 (so a whole-sample delay shifts the record exactly); the term
 *   is fmaf(w, x[i + 1] - x[i], x[i]) and the sum is fp32 in tx order.  A tx with a non-finite delay or |d fs| >= 1e8 is not
 *   fired (skipped).  The bits of out[v] do not depend on which other v share the call.  out [n_v][n_rx][n_t] float32 has the
 *   FMC's layout, so rtus_fmc_analytic, rtus_tfm and rtus_tfm_analytic take it as it is; it must not overlap fmc or delays (-1).
 *
 * Argument checks run before any HIP call: -1 for a null pointer, a non-positive size, x_lo > x_hi, a non-finite scalar, a speed
 * <= 0, a non-ascending z_if, z_a >= z_if[0], fs <= 0, an overlapping synthesis output; -5 past a limit: n_a <= 65535,
 * n_if <= RTUS_MAX_LAYERS, n_s <= 2^22 (rtus_tt_surface's), n_v <= 65535, n_rx <= 65535, n_t <= 2^28.  The _dev entries allocate
 * nothing and do not synchronise (capturable).  The host twins take host buffers, stage them through the device's arena, last
 * argument `device`.
 * Measured on MI355X: see DESIGN.md §4 (plane-wave imaging).
 * ---------------------------------------------------------------------------------------- */
int rtus_pw_layers_dev(const double *z_if, const double *c, int n_if, const double *d_angles, int n_a,
                       double x_lo, double x_hi, double z_a, const double *d_xf, const double *d_zf, int n_f,
                       double *d_tt, void *stream);
int rtus_pw_layers(const double *z_if, const double *c, int n_if, const double *angles, int n_a,
                   double x_lo, double x_hi, double z_a, const double *xf, const double *zf, int n_f,
                   double *tt, int device);
int rtus_pw_surface_dev(double x0, double dx, const double *d_zs, int n_s, double c1, double c2,
                        const double *d_angles, int n_a, double x_lo, double x_hi, double z_a,
                        const double *d_xf, const double *d_zf, int n_f, double *d_tt, double *d_x_entry,
                        void *d_workspace, size_t workspace_bytes, void *stream);
int rtus_pw_surface(double x0, double dx, const double *zs, int n_s, double c1, double c2,
                    const double *angles, int n_a, double x_lo, double x_hi, double z_a,
                    const double *xf, const double *zf, int n_f, double *tt, double *x_entry, int device);
int rtus_fmc_synth_tx_dev(const float *d_fmc, int n_tx, int n_rx, int n_t, double fs, const double *d_delays, int n_v,
                          float *d_out, void *stream);
int rtus_fmc_synth_tx(const float *fmc, int n_tx, int n_rx, int n_t, double fs, const double *delays, int n_v,
                      float *out, int device);

/* ------------------------------------------------------------------------------------------
 * Multi-view TFM: legs that reflect once off the backwall, with or without a mode conversion there.  NOT IN THE REFERENCE;
 * checked against tests/skip_numpy.py (itself checked against mpmath at 40 digits), against rtus_tt_layers on a flat profile and
 * against rtus_tt_surface at the mirrored depth when c_down = c_up.
 *
 * Conventions.  The part has a planar, horizontal backwall at depth z_back and is laterally unbounded; c_l and c_t are its
 * longitudinal and transverse speeds.  A LEG is named by its modes, read from the element towards the point: "L" and "T" are the
 * direct legs; "XY" (X, Y in {L, T}) is a skip leg: element -> couplant -> front surface -> down in mode X to the backwall ->
 * reflects -> up in mode Y to the point.  Its time is the direct time to F' = (xf, 2 z_back - zf) through the stack that has one
 * more interface at z_back (speed c_X above it, c_Y below it).  A point is valid for a skip leg only if front(xf) < zf < z_back;
 * otherwise the entry is NaN.  A VIEW "A-B" is written in propagation order: transmit leg A from the transmitter to the point,
 * then receive leg B from the point to the receiver; its image is TFM with tt_tx = leg[A] and tt_rx = leg[reverse(B)]
 * (reciprocity: path B read backwards is the element-to-point leg reverse(B)).  Through planar layers a skip leg is
 * rtus_tt_layers on the stack z_if + [z_back], c + [c_up] at the mirrored depth (composed in the Python layer).
 *
 * rtus_tt_surface_skip: a skip leg through a measured surface (the spline, grid, extent, element rules and workspace of
 *   rtus_tt_surface; c1 above the surface, c_down below it down to the backwall, c_up from the backwall up to the point).
 *   With S(x) = (x, s(x)) and B = (xb, z_back):
 *       T(x) = |E - S(x)| / c1 + T_in(S(x)),   T_in(S) = min over xb of |S - B| / c_down + |B - F'| / c_up
 *   The entry is the least T over the interior local minima of T.  It is NaN under rtus_tt_surface's element and focal-point
 *   rules, when zf >= z_back, when z_back <= max s (the whole table is NaN; this is known only on the device), and when T has no
 *   interior local minimum.
 *   Guarantee: every interior local minimum whose basin spans at least one profile segment dx centred on it is found — the basin
 *   running from the minimum to its neighbouring stationary points of T or to the ends of the extent; a minimum qualifies when
 *   each neighbouring STATIONARY point is at least dx / 2 away (an end of the extent always does).  Narrower minima may be
 *   missed; a missed minimum can only make the reported time later (or NaN), never earlier.
 *   Determinism: an entry depends only on its element, its focal point, the profile and the speeds — not on which other elements
 *   or focal points share the call (the bits of a row block or a focal-point subset are those of the whole table).
 *   x_entry [n_e][n_f] (nullable): x of the winning entry point; x_back [n_e][n_f] (nullable): x of its backwall reflection
 *   point, so that a caller can mask views whose reflection falls outside a finite part.
 *   Method: rtus_tt_surface's scan and refine.  Below the surface, with p the horizontal slowness, q_d = sqrt(1/c_down^2 - p^2),
 *   q_u = sqrt(1/c_up^2 - p^2), h1 = z_back - s(x), h2 = z_back - zf, X = xf - x, the ray solves
 *       f(p) = h1 p / q_d + h2 p / q_u - X = 0   (one root with |p| < 1 / max(c_down, c_up): h1, h2 > 0),
 *   T_in = p X + h1 q_d + h2 q_u and dT_in/dx = -(p + q_d s').  The fp32 scan takes a fixed number of safeguarded Newton steps
 *   per scan point, warm-started from the previous one; the fp64 refine solves p to convergence.
 *   Argument checks run before any HIP call, with rtus_tt_surface's codes: -1 also for a non-finite or non-positive speed or a
 *   non-finite z_back.  d_workspace: rtus_tt_surface_workspace_bytes(n_s) bytes, 256-byte aligned (-4 otherwise).
 *   Measured on MI355X: see DESIGN.md §4 (multi-view TFM).
 * ---------------------------------------------------------------------------------------- */
int rtus_tt_surface_skip_dev(double x0, double dx, const double *d_zs, int n_s, double c1, double c_down, double c_up, double z_back,
                             const double *d_xe, const double *d_ze, int n_e, const double *d_xf, const double *d_zf, int n_f,
                             double *d_tt, double *d_x_entry, double *d_x_back, void *d_workspace, size_t workspace_bytes,
                             void *stream);
int rtus_tt_surface_skip(double x0, double dx, const double *zs, int n_s, double c1, double c_down, double c_up, double z_back,
                         const double *xe, const double *ze, int n_e, const double *xf, const double *zf, int n_f,
                         double *tt, double *x_entry, double *x_back, int device);

/* ------------------------------------------------------------------------------------------
 * Ray amplitudes and sensitivity-normalised multi-view TFM (the ray model of Budyn, Bevan, Zhang, Croxford and Wilcox, IEEE UFFC
 * 2019).  NOT IN THE REFERENCE; checked against tests/amplitude_numpy.py, itself checked against a 40-digit mpmath solve of the
 * boundary conditions, energy balance, reciprocity and a finite-difference ray tube (tests/test_amplitude_cpu.py).
 *
 * Media.  Couplant: a fluid, density rho1, speed c1.  Part: an isotropic elastic solid, density rho2, speeds c_l > c_t, with a planar
 * traction-free backwall at z_back.  Front surface: rtus_tt_surface's natural cubic spline s(x), local normal n = (-s', 1) / sqrt(1 +
 * s'^2) (z points down).  Elements are horizontal and face +z.
 * Legs (the multi-view conventions above): E = (xe, ze) the element, S = (x_entry, s(x_entry)) the entry point, B = (x_back, z_back)
 * the backwall point (skip legs), F = (xf, zf) the point; x_entry / x_back are what rtus_tt_surface[_skip] return, no solve is made.
 * Direction: DOWN — the wave travels E -> S -> (B) -> F; UP — F -> (B) -> S -> E along the same path (for "XY": down in Y to the
 * backwall, up in X to the surface).  View "A-B": transmit weight from DOWN of leg A, receive weight from UP of leg reverse(B) (the
 * table the view already uses for tt_rx).
 *
 * Amplitude A = D C_S [C_B] G, formed in fp64, stored as complex64:
 *   D    directivity sinc(w sin(theta_E) / lambda1), sinc(u) = sin(pi u) / (pi u), lambda1 = c1 / f_c, theta_E the angle of E - S to
 *        +z, w the element width (w = 0: D = 1).
 *   C_S  the plane-wave DISPLACEMENT-amplitude coefficient at the surface at the local incidence angle on n: DOWN fluid -> solid into
 *        the leg's first mode; UP solid -> fluid from the mode that arrives at the surface.
 *   C_B  (skip legs) the free-surface displacement reflection coefficient, incoming mode -> outgoing mode in propagation order (DOWN
 *        X -> Y, UP Y -> X).
 *        Boundary conditions: fluid-solid — continuity of the normal displacement and of the normal traction (sigma_nn = -p), zero
 *        shear traction; backwall — zero normal and shear traction.  Polarisation: L along the propagation direction d, T along
 *        (-d_z, d_x).  The other modes may be evanescent (past a critical angle): the coefficients are complex.  Each coefficient is
 *        the horizontal slowness p of the segment that arrives at the interface.
 *   G    2-D geometric spreading of the ray tube, G = sqrt( prod_k (cos theta_out,k / cos theta_in,k) / |J| ), J = dq / dphi the tube's
 *        width at the end point (measured perpendicular to the last segment) per radian of launch angle at the start (the element
 *        DOWN, the point UP), the product over the surface crossing and the backwall reflection with angles on the local normals.
 *        Closed form: the width W and the direction change Th per launch radian start at (0, 1); a segment of length l adds l Th to W;
 *        at an interface with incidence / exit cosines ci, co, speeds c_in, c_out and normal turning at K per arc length (K = -+ s'' /
 *        (1 + s'^2)^{3/2} at the surface, for a ray going down / up; 0 at the backwall): ds = W / ci, dtin = Th - K ds, dtout = c_out ci
 *        / (c_in co) dtin, then transmission W = ds co, Th = K ds + dtout; reflection W = -ds co, Th = K ds - dtout.  J is the final W.
 *        (Homogeneous: G = 1 / sqrt(r); a flat interface: G = 1 / sqrt(r1 + r2 (c2 / c1) cos^2 theta1 / cos^2 theta2).)
 *   Phase convention: the entry is the factor that multiplies the ANALYTIC signal of the wave (rtus_fmc_analytic's positive-frequency
 *   phasor e^{+iwt}) — the complex conjugate of the coefficients as derived in the e^{i(k.x - wt)} convention.
 *   Invalid entries: NaN + NaN i exactly where x_entry (or, for skip legs, x_back) is NaN — where the time table is NaN.  A stationary
 *   path that does not cross the surface from the couplant into the part (E - S or the segment below S not pointing along +n: the
 *   time solvers do not check occlusion, and on a steep facet a point may lie above the local tangent) carries no ray: 0 + 0 i.  At
 *   a caustic (J = 0) ray theory fails and the entry is +inf + inf i (rtus_tfm_weighted drops such a leg).  An infinite x_entry or
 *   x_back names no point of the surface or the backwall: its segments have no direction, the crossing test above fails, 0 + 0 i.
 *   The path is an input and is not put to Snell's law: each coefficient is evaluated at the slowness of the segment that arrives,
 *   whatever the segment that leaves does, and every other wave of the boundary problem may be evanescent, the transmitted one
 *   included (UP with p c1 > 1, possible where c_t < c1: the coefficient is that of the evanescent wave in the couplant, finite and
 *   not zero).  Conditioning: the T coefficients vanish at p = 0 and the first-mode-T amplitude like sqrt|p c_l - 1| at the first
 *   critical angle; a segment at the cosine k on a normal has the vertical slowness k / c, formed as sqrt(1 / c^2 - p^2), which
 *   fp64 holds to 1e-16 / k^2 relative: below k = 3e-5 the entry of a grazing path is not good to 1e-7.
 *
 * rtus_leg_amp_surface: amp [n_e][n_f] complex64 (interleaved float32 pairs) of one leg in one direction.
 *   x0, dx, zs, n_s, xe, ze, xf, zf: rtus_tt_surface's; x_entry [n_e][n_f] the leg's entry points; x_back [n_e][n_f] its backwall points
 *   (skip legs; nullable for L and T).  leg: RTUS_LEG_*; direction: RTUS_AMP_DOWN / RTUS_AMP_UP; element_width >= 0 [m] and f_c > 0
 *   [Hz] (f_c is read only when element_width > 0).  Determinism: an entry depends only on its own inputs (subsets give the same bits).
 *   Argument checks run before any HIP call: -1 for a null pointer, a non-positive size, a bad leg or direction, a non-finite or
 *   non-positive speed or density, c_t >= c_l, a non-finite z_back, a negative width, f_c <= 0 with a width; -5 past n_s <= 2^22 or
 *   n_e <= 65535.  d_workspace: rtus_tt_surface_workspace_bytes(n_s) bytes, 256-byte aligned (-4 otherwise); the spline is set up in it
 *   by rtus_tt_surface's set-up kernel.
 *
 * rtus_tfm_weighted: S[f] = sum over (tx, rx) of w_tx[tx][f] w_rx[rx][f] a[tx][rx](tau_tx + tau_rx) — rtus_tfm_analytic's arguments,
 *   sample positions, interpolation, edge rules and no-path rule, plus complex64 weights w_tx [n_tx][n_f], w_rx [n_rx][n_f].  A leg
 *   whose weight is not finite also contributes nothing (it cannot poison the pixel).  image [n_f] complex64, fp32 sums: per tx the
 *   receive tiles of 16 elements are summed with their weights, then multiplied by the transmit weight.
 *   sens [n_f] float32, nullable: P[f] = (sum over tx with a path of |w_tx|^2) (sum over rx with a path of |w_rx|^2), fp32 sums, the
 *   product in fp64 rounded once.  With w = conj(A) (A the leg amplitudes), P is the sensitivity — the image at f of a unit isotropic
 *   point scatterer at f — and |S| / P reads the scatterer's own amplitude; views become comparable.  Passing sens does not change the
 *   bits of image; the bits of a focal point do not depend on which other focal points share the call.
 *   Limits and codes: rtus_tfm_analytic's (w_tx, w_rx required, sens nullable).
 *
 * The _dev entries allocate nothing and do not synchronise (capturable); the host twins stage through the device's arena.
 * Measured on MI355X: see DESIGN.md §4 (ray amplitudes).
 * ---------------------------------------------------------------------------------------- */
enum { RTUS_LEG_L = 0, RTUS_LEG_T = 1, RTUS_LEG_LL = 2, RTUS_LEG_LT = 3, RTUS_LEG_TL = 4, RTUS_LEG_TT = 5 };
enum { RTUS_AMP_DOWN = 0, RTUS_AMP_UP = 1 };
int rtus_leg_amp_surface_dev(double x0, double dx, const double *d_zs, int n_s, double c1, double rho1, double c_l, double c_t,
                             double rho2, double z_back, int leg, int direction, double element_width, double f_c,
                             const double *d_xe, const double *d_ze, int n_e, const double *d_xf, const double *d_zf, int n_f,
                             const double *d_x_entry, const double *d_x_back, float *d_amp, void *d_workspace, size_t workspace_bytes,
                             void *stream);
int rtus_leg_amp_surface(double x0, double dx, const double *zs, int n_s, double c1, double rho1, double c_l, double c_t,
                         double rho2, double z_back, int leg, int direction, double element_width, double f_c,
                         const double *xe, const double *ze, int n_e, const double *xf, const double *zf, int n_f,
                         const double *x_entry, const double *x_back, float *amp, int device);
int rtus_tfm_weighted_dev(const float *d_a, int n_tx, int n_rx, int n_t, double fs, double t0,
                          const double *d_tt_tx, const double *d_tt_rx, const float *d_w_tx, const float *d_w_rx, int n_f,
                          float *d_image, float *d_sens, void *stream);
int rtus_tfm_weighted(const float *a, int n_tx, int n_rx, int n_t, double fs, double t0,
                      const double *tt_tx, const double *tt_rx, const float *w_tx, const float *w_rx, int n_f,
                      float *image, float *sens, int device);

/* ------------------------------------------------------------------------------------------
 * Element x focal-point travel times from elements behind the curved lens INTO THE PIPE WALL: two curved refractions, the lens
 * surface and then the pipe's outer circle.  NOT IN THE REFERENCE (it defines the wall speed c3 = 5600 and never uses it); checked
 * against tests/pipe_numpy.py, itself checked against a 40-digit joint solve in (alpha, beta) (tests/test_pipe_cpu.py).
 *
 * Geometry is the reference's (z up, elements in the lens at ze, normally d): lens surface P(alpha) = h(alpha)(sin alpha, cos alpha)
 * (rtus_tt_lens's), pipe centre Cp = (x_off, 0), outer surface Q(beta) = (x_off + r_outer sin beta, r_outer cos beta) (the angle of
 * main_rt.py:250-252).  The wall is r_inner < |F - Cp| < r_outer, 0 <= r_inner < r_outer (0: a solid bar).
 *     T(beta)      = T_lens(E, Q(beta)) + |Q(beta) - F| / c3
 *     T_lens(E, Q) = rtus_tt_lens's entry for the target Q: the least time over alpha in [alpha_lo, alpha_hi], pinned ends included
 *     tt[e][f]     = the least T over the interior local minima of T on (beta_lo, beta_hi) whose path qualifies:
 *       1. the water segment L(alpha*) -> Q arrives from outside the circle, (Q - L) . (Q - Cp) < 0;
 *       2. the wall segment Q -> F keeps a distance of at least r_inner from Cp (it does not cross the bore).
 * NaN for an F outside the wall, without a qualifying interior minimum (total reflection past the critical angle included), and for
 * the rows of elements with a non-finite position.  alpha_out, beta_out [n_e][n_f] (nullable): the lens refraction point's and the
 * pipe entry point's angles.
 * Guarantee: beta_lo .. beta_hi is scanned at n_scan equally spaced points; every interior local minimum whose neighbouring
 * stationary points of T(beta) lie at least one scan step away is found.  A missed minimum can only make an entry later (or NaN),
 * never earlier.  The three earliest minima (by an fp32 estimate of T) are kept; each is refined and put to rules 1-2 in turn, the
 * third however late it is while the first two were rejected, and otherwise when its estimate is within 4e-6 of the qualifying
 * one's.  A fourth minimum is never looked at (none of the tested geometries has one: tests/test_gpu_pipe_branches.py).
 * Determinism: an entry depends only on its element, its focal point and the parameters, not on which other elements or points
 * share the call.
 * Rejected: a pipe that touches the lens, r_outer >= min over alpha in [alpha_lo, alpha_hi] of |P(alpha) - Cp| (RTUS_ERR_INVALID_ARG,
 * checked on the host before any HIP call).
 * Argument checks run before any HIP call: -1 for a null pointer, a non-positive size, a speed that is not finite and positive,
 * r_inner outside [0, r_outer), non-finite x_off or interval ends, alpha_lo >= alpha_hi, beta_lo >= beta_hi, n_scan < 4 or a pipe
 * touching the lens; -5 past n_e <= 65535 * 8, n_scan <= 65536, n_e * n_scan <= 2^26.  d_workspace:
 * rtus_tt_pipe_workspace_bytes(n_e, n_scan) bytes, 256-byte aligned (-4 otherwise; the function returns 0 for sizes it rejects).
 * The _dev entry allocates nothing and does not synchronise (capturable); the host twin stages through the device's arena.
 * Method and measured figures on MI355X: DESIGN.md section 4 (pipe wall).
 * ---------------------------------------------------------------------------------------- */
typedef struct rtus_pipe {
    double r_outer; /* outer radius [m]                       main_rt.py:466 */
    double r_inner; /* bore radius [m], 0 <= r_inner < r_outer (0: a solid bar) */
    double x_off;   /* x of the pipe's centre [m]             main_rt.py:467 (pipe_offset) */
    double c3;      /* speed in the wall [m/s]                main_rt.py:451 */
} rtus_pipe;
size_t rtus_tt_pipe_workspace_bytes(int n_e, int n_scan);
int rtus_tt_pipe_dev(const rtus_lens *lens, double alpha_lo, double alpha_hi, const rtus_pipe *pipe,
                     double beta_lo, double beta_hi, int n_scan,
                     const double *d_xe, const double *d_ze, int n_e, const double *d_xf, const double *d_zf, int n_f,
                     double *d_tt, double *d_alpha_out, double *d_beta_out,
                     void *d_workspace, size_t workspace_bytes, void *stream);
int rtus_tt_pipe(const rtus_lens *lens, double alpha_lo, double alpha_hi, const rtus_pipe *pipe,
                 double beta_lo, double beta_hi, int n_scan,
                 const double *xe, const double *ze, int n_e, const double *xf, const double *zf, int n_f,
                 double *tt, double *alpha_out, double *beta_out, int device);

/* ------------------------------------------------------------------------------------------
 * BORE-REFLECTED SKIP LEG into the pipe wall: the half-skip leg of multi-view TFM (LL, LT, TL, TT) for rtus_tt_pipe's geometry.
 * NOT IN THE REFERENCE; checked against tests/pipe_skip_numpy.py, itself checked against a 40-digit joint solve in (alpha, beta,
 * gamma) (tests/test_pipe_skip_cpu.py).
 *
 * Geometry and symbols are rtus_tt_pipe's; new is the reflection point on the bore, R(gamma) = Cp + r_inner (sin gamma, cos gamma).
 * A skip path is E -> P(alpha) -> Q(beta) -> R(gamma) -> F:
 *     T(beta) = T_lens(E, Q(beta)) + W(Q(beta), F)
 *     W(Q, F) = min over gamma of |Q - R(gamma)| / c_down + |R(gamma) - F| / c_up
 * c_down = pipe->c3 is the wall speed before the bounce, c_up the speed after it (a different speed: a mode conversion at the bore).
 * T_lens is rtus_tt_pipe's lens leg.  gamma runs over the arc of the bore that Q and F both see, (Q - R) . (R - Cp) > 0 and
 * (F - R) . (R - Cp) > 0: both wall segments leave R outwards, touch the convex bore nowhere else and stay inside the outer circle.
 * W is the time at the interior local minimum on that arc.  On the arc both lengths are convex functions of gamma
 * (d2|Q - R| / dgamma2 = r_outer r_inner (r_outer cos u - r_inner)(r_outer - r_inner cos u) / |Q - R|^3, u = gamma - beta, which
 * is positive exactly where Q sees R; likewise for F), so for any pair of speeds there is at most one such minimum.  Where the arc is
 * empty or the least time sits at an end of it (a grazing bounce; past the critical angle of a T -> L conversion) there is no W: such
 * a beta is neither side of a bracket, as an element without a lens leg is in rtus_tt_pipe.
 *     tt[e][f] = the least T over the interior local minima of T on (beta_lo, beta_hi) whose path satisfies rtus_tt_pipe's rule 1.
 * NaN for an F not strictly inside the wall, for a non-finite element position and where no minimum qualifies.  alpha_out, beta_out,
 * gamma_out [n_e][n_f] (nullable): the angles of the lens point, the entry point and the bounce (gamma = beta + u, not wrapped).
 * Guarantee and selection among the three earliest minima: rtus_tt_pipe's; a minimum closer than one scan step to a beta without W
 * may be missed as one closer than a scan step to another stationary point may.  Determinism: an entry depends only on its element,
 * its focal point and the parameters.
 * Rejected with RTUS_ERR_INVALID_ARG: everything rtus_tt_pipe rejects, r_inner <= 0 (no bore, no skip leg) and a c_up that is not
 * finite and positive.  Limits (-5) and the workspace (-4; rtus_tt_pipe_skip_workspace_bytes, 256-byte aligned) as rtus_tt_pipe's.
 * The _dev entry allocates nothing and does not synchronise (capturable).  Method and figures: DESIGN.md section 4 (pipe wall).
 * ---------------------------------------------------------------------------------------- */
size_t rtus_tt_pipe_skip_workspace_bytes(int n_e, int n_scan);
int rtus_tt_pipe_skip_dev(const rtus_lens *lens, double alpha_lo, double alpha_hi, const rtus_pipe *pipe, double c_up,
                          double beta_lo, double beta_hi, int n_scan,
                          const double *d_xe, const double *d_ze, int n_e, const double *d_xf, const double *d_zf, int n_f,
                          double *d_tt, double *d_alpha_out, double *d_beta_out, double *d_gamma_out,
                          void *d_workspace, size_t workspace_bytes, void *stream);
int rtus_tt_pipe_skip(const rtus_lens *lens, double alpha_lo, double alpha_hi, const rtus_pipe *pipe, double c_up,
                      double beta_lo, double beta_hi, int n_scan,
                      const double *xe, const double *ze, int n_e, const double *xf, const double *zf, int n_f,
                      double *tt, double *alpha_out, double *beta_out, double *gamma_out, int device);

/* ------------------------------------------------------------------------------------------
 * RAY AMPLITUDES OF THE LEGS INTO THE PIPE WALL: rtus_leg_amp_surface's table for rtus_tt_pipe's / rtus_tt_pipe_skip's geometry, so
 * that rtus_tfm_weighted images the pipe wall in sensitivity-normalised views.  NOT IN THE REFERENCE; checked against
 * tests/pipe_amplitude_numpy.py, itself checked against a finite-difference ray tube through the three curved interfaces, a
 * closed-form point on the axis, reciprocity and mirror symmetry (tests/test_pipe_amplitude_cpu.py).
 *
 * Geometry and symbols are rtus_tt_pipe's / rtus_tt_pipe_skip's (z up, elements at ze, normally d, above the lens surface and facing
 * -z; P(alpha), Q(beta), R(gamma), Cp = (x_off, 0)).  A path is E -> P(alpha) -> Q(beta) -> [R(gamma)] -> F; alpha, beta, gamma are
 * what rtus_tt_pipe[_skip] return, no solve is made.  Direction and views: the surface section's (DOWN E -> F, UP F -> E).
 * Media: the lens is an isotropic solid (rho_lens, L speed lens->c1, shear speed ct_lens, 0 < ct_lens < c1; only its L wave is
 * traced); water (rho_water, lens->c2); the wall (rho_wall, c_l > c_t); the bore is traction-free.
 *
 * Amplitude A = conj(D C_lens C_outer [C_bore] G), formed in fp64, stored as complex64, with the surface section's conventions:
 * component algebra in (x, z) exactly as written there (polarisation L along the propagation direction d, T along (-d_z, d_x); an
 * interface frame is a unit normal n with the tangent t = (n_z, -n_x), the horizontal slowness p is taken along t; angles grow from
 * +z towards +x), derivation in e^{i(k.x - wt)}, the conjugate stored.
 *   D        sinc(w sin(theta_E) f_c / c1), theta_E the angle of P - E to the element's facing direction; w = 0: D = 1.
 *   C_lens   DOWN solid -> fluid from L, UP fluid -> solid into L, the lens being the solid.  Frame: n into the lens, t = P' / |P'|.
 *   C_outer  DOWN fluid -> solid into the leg's first mode, UP solid -> fluid from the mode that arrives at Q.  Frame: n into the
 *            wall, n = -(Q - Cp) / r_outer.
 *   C_bore   (skip legs) free-surface reflection, incoming -> outgoing mode in propagation order.  Frame: n out of the wall,
 *            n = -(R - Cp) / r_inner.
 *            Each coefficient is evaluated at the horizontal slowness of the segment that arrives at the interface.
 *   G        the surface section's ray tube, sqrt(prod_k (cos theta_out,k / cos theta_in,k) / |J|), through three (direct) or four
 *            (skip) segments.  Tube normals and their turning rates K = d(angle of n) / d(arc along t), before the tube orients each
 *            along the incoming ray (which flips K with it): the lens n = (P'_z, -P'_x) / |P'| (towards the water),
 *            K = (P'_x P''_z - P'_z P''_x) / |P'|^3, the signed curvature of P(alpha); the outer circle n = (Q - Cp) / r_outer,
 *            K = 1 / r_outer; the bore n = (R - Cp) / r_inner, K = 1 / r_inner.
 *   Mirror rule: mirroring x_off, the elements and the points in x (alpha, beta, gamma change sign) keeps |A|; A changes sign
 *   exactly when the mode at F is T (the T polarisation (-d_z, d_x) is a pseudovector).
 *   Invalid entries: NaN + NaN i exactly where alpha or beta (or, for skip legs, gamma) is NaN — where the time table is NaN.
 *   0 + 0 i where the path is not a ray: the lens leg is pinned (alpha equal to alpha_lo or alpha_hi, which the time kernels return
 *   bit-exactly), or a segment does not cross its interface in the propagating sense ((P - E) . n and (Q - P) . n not both positive on
 *   the lens normal; (Q - P) or the wall segment from Q not pointing into the circle; for skip legs the segment to R not pointing
 *   into the bore or the segment from R not pointing out of it).  +inf + inf i at a caustic (J = 0; rtus_tfm_weighted drops it).
 *
 * rtus_leg_amp_pipe: amp [n_e][n_f] complex64 (interleaved float32 pairs) of one leg in one direction.
 *   lens, alpha_lo, alpha_hi, pipe (r_outer, r_inner, x_off; c3 is not read), xe, ze, xf, zf: rtus_tt_pipe's; alpha, beta [n_e][n_f] and
 *   gamma [n_e][n_f] (skip legs; nullable for L and T): the path.  leg: RTUS_LEG_*; direction: RTUS_AMP_*; element_width >= 0 [m]
 *   and f_c > 0 [Hz] (read only with a width).  Determinism: an entry depends only on its own inputs (subsets give the same bits).
 *   Argument checks run before any HIP call: -1 for a null pointer, a non-positive size, a bad leg or direction, a non-finite or
 *   non-positive speed or density, c_t >= c_l, ct_lens >= c1, a non-finite or non-positive r_outer, a non-finite x_off, r_inner
 *   outside [0, r_outer) or r_inner = 0 with a skip leg, alpha_lo >= alpha_hi, a negative width, f_c <= 0 with a width, a skip leg
 *   without gamma; -5 past n_e <= 65535.  No workspace.
 * The _dev entry allocates nothing and does not synchronise (capturable); the host twin stages through the device's arena.
 * Kernel, resources and measured figures on MI355X: DESIGN.md section 4 (pipe wall, ray amplitudes).
 * ---------------------------------------------------------------------------------------- */
typedef struct rtus_pipe_media {
    double rho_lens;  /* density of the lens [kg/m^3] */
    double ct_lens;   /* shear speed of the lens [m/s], 0 < ct_lens < lens->c1 */
    double rho_water; /* density of the water [kg/m^3] */
    double rho_wall;  /* density of the wall [kg/m^3] */
    double c_l;       /* L speed of the wall [m/s] */
    double c_t;       /* T speed of the wall [m/s], c_t < c_l */
} rtus_pipe_media;
int rtus_leg_amp_pipe_dev(const rtus_lens *lens, double alpha_lo, double alpha_hi, const rtus_pipe *pipe, const rtus_pipe_media *media,
                          int leg, int direction, double element_width, double f_c,
                          const double *d_xe, const double *d_ze, int n_e, const double *d_xf, const double *d_zf, int n_f,
                          const double *d_alpha, const double *d_beta, const double *d_gamma, float *d_amp, void *stream);
int rtus_leg_amp_pipe(const rtus_lens *lens, double alpha_lo, double alpha_hi, const rtus_pipe *pipe, const rtus_pipe_media *media,
                      int leg, int direction, double element_width, double f_c,
                      const double *xe, const double *ze, int n_e, const double *xf, const double *zf, int n_f,
                      const double *alpha, const double *beta, const double *gamma, float *amp, int device);

/* ------------------------------------------------------------------------------------------
 * Estimating the pipe's geometry (r_outer, pipe_offset) from measured echo times: pick the outer-surface echo of every pair of an
 * FMC (rtus_echo_pick), then compare the picks with rtus_solve's times for a batch of geometries (rtus_geom_misfit) — the
 * reference's database search (main_rt.py:464-504 tabulates 210 geometries, main_compare.py:526-553 takes the one of least mean
 * squared error) on any batch, which the Python layer (api.pipe_misfit, api.fit_pipe) turns into a coarse map and a
 * Levenberg-Marquardt refinement.  The kernels are NOT IN THE REFERENCE; checked against tests/geomfit_numpy.py.
 *
 * rtus_echo_pick: the time of the strongest echo inside a gate, for every pair.
 *   a        [n_tx][n_rx][n_t][2]  an analytic FMC as rtus_fmc_analytic makes it (8-byte aligned, -1 otherwise); sample i is at
 *                                  t0 + i / fs
 *   gate     the samples i with t_lo <= t0 + i / fs <= t_hi, formed as i_lo = ceil((t_lo - t0) fs), i_hi = floor((t_hi - t0) fs) in
 *            fp64 and cut to the record [0, n_t - 1].  t_lo / t_hi are either the two scalars or, where the pointer is not null,
 *            the pair's entry of d_t_lo / d_t_hi [n_tx][n_rx] (fp64; DEVICE memory in the _dev entry); each array wins over its
 *            scalar on its own.  An infinite bound leaves that side open.
 *   Magnitude: m[i] = sqrt(re * re + im * im) in fp32, each of the four operations correctly rounded on its own (no fused
 *            multiply-add, no approximate root).
 *   Pick:    j* = the first index of the maximum of m over the gate.  t_pick = NaN when j* is the first or the last sample of the
 *            gate, when the maximum is 0 or not finite, when the gate is empty (a NaN bound included) or lies outside the record;
 *            otherwise t0 + (j* + d) / fs with rtus_surface_find's parabolic step d = (m- - m+) / (2 (m- - 2 m0 + m+)) over
 *            m[j* - 1 .. j* + 1] in fp64, clamped to [-1/2, 1/2].
 *   Outputs: t_pick [n_tx][n_rx] fp64; amp [n_tx][n_rx] float32 = m[j*] (NaN when the gate is empty or holds a non-finite
 *            magnitude).
 *   Determinism: a pair's bits depend only on its own A-scan and gate, not on the other pairs of the call nor on the block's
 *            alignment.
 *   Limits:  n_t >= 3, fs > 0 and finite, t0 finite, a scalar bound that is read not NaN (-1); n_t <= 2^26, n_tx n_rx <= 2^31 - 1
 *            (-5); checked before any HIP call.  No workspace.
 *
 * rtus_geom_misfit: sums of the residuals tt[g] - t_meas for every geometry of a batch.
 *   tt       [n_geom][n_tx][n_rx]  rtus_solve's least times (NaN: no path)
 *   t_meas   [n_tx][n_rx]          measured times (NaN: no measurement);  w [n_tx][n_rx] weights, nullable (then 1)
 *   A pair counts for geometry g where tt[g] and t_meas are both finite and w > 0.  Over those pairs, with r = tt[g] - t_meas:
 *     n[g] = their number,  sse[g] = sum w r^2,  sum_r[g] = sum w r,  sum_w[g] = sum w (nullable output).
 *   A common time offset (a wedge delay, a trigger offset) then follows in closed form: delay = -sum_r / sum_w removes it, and the
 *   sum of squares without it is sse - sum_r^2 / sum_w.  With unit weights and one transmit row, sse / n is the reference's mse.
 *   Order of the sums (fp64): within a transmit row the receive elements in ascending order, q = fma(w r, r, q) for sse; then the
 *   row sums in ascending row order.  A geometry's bits do not depend on which other geometries share the call.
 *   n[g] = 0 and zero sums for a geometry without a counting pair.
 *   Limits:  n_tx n_rx <= 2^31 - 1 (-5); null pointers and non-positive sizes -1; before any HIP call.  No workspace.
 *
 * rtus_pipe_clearance: the least distance from (x_off, 0) to the lens surface over [alpha_lo, alpha_hi] — rtus_tt_pipe rejects a
 *   pipe whose r_outer is not below it.  Host arithmetic only; NaN for invalid arguments.
 * The _dev entries allocate nothing and do not synchronise (capturable); the host twins stage through the device's arena.
 * Kernels, resources and measured figures on MI355X: DESIGN.md section 4 (pipe geometry from echo times).
 * ---------------------------------------------------------------------------------------- */
int rtus_echo_pick_dev(const float *d_a, int n_tx, int n_rx, int n_t, double fs, double t0, double t_lo, double t_hi,
                       const double *d_t_lo, const double *d_t_hi, double *d_t_pick, float *d_amp, void *stream);
int rtus_echo_pick(const float *a, int n_tx, int n_rx, int n_t, double fs, double t0, double t_lo, double t_hi,
                   const double *t_lo_pair, const double *t_hi_pair, double *t_pick, float *amp, int device);
int rtus_geom_misfit_dev(const double *d_tt, int n_geom, int n_tx, int n_rx, const double *d_t_meas, const double *d_w,
                         int *d_n, double *d_sse, double *d_sum_r, double *d_sum_w, void *stream);
int rtus_geom_misfit(const double *tt, int n_geom, int n_tx, int n_rx, const double *t_meas, const double *w,
                     int *n, double *sse, double *sum_r, double *sum_w, int device);
double rtus_pipe_clearance(const rtus_lens *lens, double alpha_lo, double alpha_hi, double x_off);

/* ------------------------------------------------------------------------------------------
 * THE FORWARD MODEL: arrivals to the A-scans of a full-matrix capture (FMC) — the way back from the tables of this library to
 * data.  rtus_tfm_weighted with w = conj(A) is the matched filter of this model.  NOT IN THE REFERENCE; checked against
 * tests/fmcsim_numpy.py (the same formulas with fp64 sums).
 *
 * Every arrival, a time tau and a complex amplitude a, adds a p(t_j - tau) to the samples t_j = t0 + j / fs, 0 <= j < n_t, of
 * its A-scan.  Two ways of stating the arrivals, one kernel body:
 *   rtus_fmc_sim       scatterer s arrives in A-scan (tx, rx) at tau = tt_tx[tx][s] + tt_rx[rx][s] (one fp64 sum) with
 *                      a = (q[s] w_tx[tx][s]) w_rx[rx][s].
 *                        tt_tx [n_tx][n_s], tt_rx [n_rx][n_s]  fp64; any table of this library; the two may be one table
 *                        q [n_s], w_tx [n_tx][n_s], w_rx [n_rx][n_s]  complex64 (interleaved float32 pairs, 8-byte aligned), each
 *                        nullable: null is the factor 1 (that product is skipped)
 *   rtus_fmc_sim_echo  arrival k of pair (tx, rx) is given directly: tau = t_pair[tx][rx][k], a = amp[tx][rx][k]
 *                        t_pair [n_tx][n_rx][n_a] fp64 (n_a >= 1; e.g. rtus_solve's tt, n_a = 1); amp complex64, nullable (1)
 *   A complex product is (ar br - ai bi, ar bi + ai br) in fp32, every operation rounded on its own.
 *
 * The wavelet p is a table: pulse [n_p] complex64 sampled at fs * oversample (oversample an integer >= 1), time zero at index
 * `centre`.  The table continues with p[-1] = p[n_p] = 0 and is zero beyond; between samples it is interpolated linearly, the real
 * and the imaginary part separately, each as fmaf(w, p[i + 1] - p[i], p[i]) with the difference rounded to fp32 (rtus_tfm_analytic's
 * rule).  The values of the table are expected to be finite.
 * Position (PINNED; fp64, every operation rounded on its own, no fused multiply-add):
 *     d  = ((tau - t0) * fs) * oversample          the arrival in table steps after the record's start
 *     x0 = centre - d                              the table position of sample 0
 *     i0 = floor(x0),  w = (float)(x0 - i0)        (the difference is exact; w is rounded once)
 *   sample j reads the table at i = i0 + j * oversample with the weight w — the same w for every sample of the arrival; it is
 *   touched iff -1 <= i <= n_p - 1.  An arrival contributes NOTHING when its time is not finite or |d| >= 2^30, or when q, w_tx,
 *   w_rx / amp or their product has a non-finite part: it never poisons the A-scan.  Samples before 0 or at / past n_t are dropped,
 *   the rest of the pulse is still written.
 * Sample update, with (pr, pi) the interpolated wavelet and (ar, ai) the amplitude:
 *     re = fmaf(-ai, pi, fmaf(ar, pr, re)),   im = fmaf(ai, pr, fmaf(ar, pi, im))
 *
 * out  [n_tx][n_rx][n_t] float32: the real part; with RTUS_SIM_ANALYTIC complex64 [n_tx][n_rx][n_t][2] (the real parts of the two
 *      are the same bits).  Without RTUS_SIM_ACCUMULATE the call zeroes out itself (what out held is never read); with it, the
 *      arrivals are added onto what out holds.
 * ACCUMULATION CONTRACT (tested by bits):
 *   - a sample's real and imaginary sums are fp32; its arrivals are added strictly in ascending s (or k), starting from the
 *     sample's initial value (0, or what out held);
 *   - the bits of an A-scan depend only on its own rows of the inputs and the scalars: any subset of tx or rx rows reproduces them;
 *   - one call over n_s scatterers equals, bit for bit, a call over the first m followed by a RTUS_SIM_ACCUMULATE call over the rest:
 *     reflector sets of any size can be streamed in chunks.  A multi-view FMC is such a chain, one call per view in the order the
 *     caller states (api.simulate_views: the views in the order given, "A-B" before its reciprocal "B-A");
 *   - host twin, _dev twin and a captured-graph replay give the same bits.
 * Argument checks run before any HIP call: -1 for a null required pointer (the time tables, pulse, out), a non-positive size,
 *   fs not finite and positive, t0 not finite, oversample < 1, centre outside [0, n_p), an unknown flag bit, a complex64 array that
 *   is not 8-byte aligned or an out that is not 4-byte aligned; -5 past n_t <= 2^26, n_p + oversample <= 2048 (the wavelet's 16-byte
 *   entries take half of a workgroup's 64 KB of LDS), n_tx n_rx ceil(n_t / 1024) <= 2^31 - 1.  No workspace.
 * The _dev entries allocate nothing and do not synchronise (capturable); the host twins stage through the device's arena (one
 * table uploaded when tt_tx == tt_rx, out uploaded only with RTUS_SIM_ACCUMULATE).
 * Kernel, resources and measured figures on MI355X: DESIGN.md section 4 (FMC simulator).
 * ---------------------------------------------------------------------------------------- */
#define RTUS_SIM_ANALYTIC 0x1u
#define RTUS_SIM_ACCUMULATE 0x2u
int rtus_fmc_sim_dev(const double *d_tt_tx, const double *d_tt_rx, int n_tx, int n_rx, int n_s,
                     const float *d_q, const float *d_w_tx, const float *d_w_rx,
                     const float *d_pulse, int n_p, int centre, int oversample, double fs, double t0, int n_t,
                     float *d_out, unsigned flags, void *stream);
int rtus_fmc_sim(const double *tt_tx, const double *tt_rx, int n_tx, int n_rx, int n_s,
                 const float *q, const float *w_tx, const float *w_rx,
                 const float *pulse, int n_p, int centre, int oversample, double fs, double t0, int n_t,
                 float *out, unsigned flags, int device);
int rtus_fmc_sim_echo_dev(const double *d_t_pair, const float *d_amp, int n_tx, int n_rx, int n_a,
                          const float *d_pulse, int n_p, int centre, int oversample, double fs, double t0, int n_t,
                          float *d_out, unsigned flags, void *stream);
int rtus_fmc_sim_echo(const double *t_pair, const float *amp, int n_tx, int n_rx, int n_a,
                      const float *pulse, int n_p, int centre, int oversample, double fs, double t0, int n_t,
                      float *out, unsigned flags, int device);

/* ------------------------------------------------------------------------------------------
 * rtus_tfm_phase: phase-coherence imaging (Camacho, Parrilla & Fritsch 2009, "PCI") — rtus_tfm_analytic's delay-and-sum and, per
 * focal point, two factors that read only the PHASE of the aperture data: the vector coherence factor vcf and the sign coherence
 * factor scf.  Both ignore amplitude (saturated echoes, gain differences between elements, the dynamic range of multi-view
 * images), which rtus_tfm_analytic's cf does not.  NOT IN THE REFERENCE; checked against tests/tfm_phase_numpy.py.
 *   a, fs, t0, tt_tx, tt_rx, n_f: exactly as in rtus_tfm_analytic — the same sample positions (fp32 legs, s = tau_tx + tau_rx,
 *           i = floor(s), w = s - i), edge rules and accumulation order (receive tiles of 64 elements, then tx ascending, then rx
 *           ascending inside the tile).  For focal point f let p_k be the interpolated complex sample of pair k, each part
 *           fmaf(w, x[i + 1] - x[i], x[i]); p_k = 0 for a pair without a path or with a position outside the record.
 *   image   [n_f][2]  S = sum p_k: BIT-IDENTICAL to rtus_tfm_analytic's image, whichever of the other outputs are asked for.
 *   N = T R, rtus_tfm_analytic's count (T, R: the tx and rx legs with a path at f).  A pair with a path whose position falls
 *           outside the record counts in N with a zero phasor and a zero sign (cf's convention).
 *   U = sum u_k, the sum of unit phasors: u_k = p_k / |p_k|, and u_k = 0 exactly when both parts of p_k are zero.  u_k is a unit
 *           phasor to a few fp32 ulp for EVERY non-zero finite fp32 p_k, also where |p_k|^2 would under- or overflow in fp32
 *           (|p| ~ 1e-30, 1e30): both parts are scaled by the power of two 2^-e, e the exponent of max(|re|, |im|) (exact), then
 *           multiplied by one reciprocal square root of the scaled squared modulus.  U is accumulated in fp32 in the fixed order.
 *   B = sum sign(Re p_k), sign in {-1, 0, +1}: an int32, exact.
 *   vcf     [n_f] float32, nullable.  vcf = |U| / N, formed in fp64 from the fp32 sums, clamped to [0, 1], rounded once to fp32;
 *           NaN when N = 0.  The circular coherence factor of the same paper is 1 - sqrt(1 - vcf^2) when every pair has a non-zero
 *           sample (the circular variance of the phases is then 1 - vcf^2).
 *   scf     [n_f] float32, nullable.  scf = 1 - sqrt(1 - (B / N)^2), formed in fp64, rounded once to fp32; NaN when N = 0.
 *   counts  [n_f][2] int32, nullable: (B, N).
 *           A weighted image is |S| vcf^p or |S| scf^p, the exponent the caller's choice.  An output that is not asked for costs
 *           nothing in the gather loop.  Non-finite samples in a are the caller's error.
 *   Determinism: as rtus_tfm_analytic — the bits of a focal point depend only on its own columns of the tables; no output's bits
 *           depend on which other outputs are asked for.
 *   Limits: rtus_tfm_analytic's (image required; vcf, scf, counts nullable) and n_tx n_rx <= 2^30 (the sign sum is an int32): -1
 *           for invalid arguments, -5 past a limit, before any HIP call.  The _dev entry allocates nothing and does not
 *           synchronise (capturable).  The host twin stages through the arena as rtus_tfm_analytic does (one table uploaded when
 *           tt_tx == tt_rx, only the outputs asked for downloaded).
 * Measured on MI355X (CUDA-event timing, rtus_tfm_analytic_dev without cf in the same run = 1): 64 elements x 2048
 * samples, 256^2 focal points: image alone 269 us (1.00x of 268 us), vcf 287 us (1.07x), scf 268 us (1.00x), counts 269 us (1.00x),
 * vcf + scf 305 us (1.14x), all outputs 303 us (1.13x); 1024^2: image alone 1.91 ms (1.00x of 1.91 ms), vcf 2.70 ms (1.42x), scf
 * 2.03 ms (1.07x), counts 2.03 ms (1.06x), vcf + scf 3.01 ms (1.58x), all outputs 3.01 ms (1.58x).
 * ---------------------------------------------------------------------------------------- */
int rtus_tfm_phase_dev(const float *d_a, int n_tx, int n_rx, int n_t, double fs, double t0,
                       const double *d_tt_tx, const double *d_tt_rx, int n_f,
                       float *d_image, float *d_vcf, float *d_scf, int *d_counts, void *stream);
int rtus_tfm_phase(const float *a, int n_tx, int n_rx, int n_t, double fs, double t0,
                   const double *tt_tx, const double *tt_rx, int n_f,
                   float *image, float *vcf, float *scf, int *counts, int device);

/* ------------------------------------------------------------------------------------------
 * rtus_specular: specular echo times of sampled reflectors.  The echo of a reflecting boundary for transmitter i and receiver k
 * arrives at the stationary value, over the points P of the boundary, of t(i -> P) + t(P -> k) (Fermat).  Every table entry of this
 * library gives t(element -> P) for arbitrary points — through layers, a measured surface, the lens and the pipe — so the echo
 * times of a boundary sampled at n_p points, for every pair and for a batch of n_refl candidate boundaries, are a reduction over
 * two tables: a min-plus product with sub-sample refinement.  The Python layer builds on it the backwall echo under layers and
 * under a measured surface, the echo of the pipe's bore, and one-parameter fits of the backwall depth and the bore radius
 * (api.backwall_echo_layers, backwall_echo_surface, bore_echo_pipe, fit_reflector, measure_reflector).  NOT IN THE REFERENCE;
 * checked bit for bit against tests/specular_numpy.py.
 *   tt_a    [n_a][n_refl n_p]  times from the n_a transmitters; reflector g owns columns [g n_p, (g + 1) n_p), its points in
 *                              order along the reflector — the shape a table call over the concatenated points of all
 *                              candidates returns
 *   tt_b    [n_b][n_refl n_p]  times to the n_b receivers; NULL: tt_a, and then n_b must equal n_a (-1 otherwise)
 *   t       [n_refl][n_a][n_b] echo times (rtus_geom_misfit's tt);  pos [n_refl][n_a][n_b] fp64, nullable: the reflection point
 *                              in units of the point index;  n_min [n_refl][n_a][n_b] int32, nullable
 * Definition, for reflector g, transmitter i, receiver k:
 *   S_j = tt_a[i][g n_p + j] + tt_b[k][g n_p + j], one fp64 addition.  S_j is FINITE when isfinite(S_j).
 *   No S_j finite: t = pos = NaN, n_min = 0.
 *   j* = the FIRST index attaining the least finite S_j.
 *   n_min = the number of j in [1, n_p - 2] with S_(j-1), S_j, S_(j+1) all finite, S_j < S_(j-1) and S_j < S_(j+1).  A diagnostic:
 *           above 1, two reflection paths compete.
 *   j* = 0 or j* = n_p - 1, or a neighbour of j* not finite: t = NaN, pos = (double) j* — the reflection point is not bracketed by
 *           the sampled span (rtus_echo_pick's convention at its gate's ends).
 *   Otherwise, with a = S_(j*-1), b = S_(j*), c = S_(j*+1), in exactly this order and every operation rounded on its own (no
 *           fused multiply-add; the division correctly rounded):
 *             d1 = a - c;  d2 = (a - b) + (c - b);  delta = 0.5 d1 / d2;  t = b - (0.25 d1) delta;  pos = j* + delta.
 *           a > b because j* is the first minimum, so d2 > 0 and |delta| <= 1/2.
 *   n_p < 3 is legal: every pair comes out NaN by the rules above.
 *   Accuracy: the parabola's value error is fourth order in the point spacing (a flat reflector 20 mm under 16 elements, +-12 mm
 *           of points: 6.7e-13 s at 33 points, 1.6e-16 s at 257).
 *   Determinism: a pair's bits depend only on its own row of tt_a and of tt_b — not on the other pairs or reflectors of the
 *           call, nor on the launch shape.  With tt_b NULL (or tt_a passed twice) t, pos and n_min are symmetric in (i, k) bit
 *           for bit.
 *   Limits: null tt_a or t, a size <= 0: -1; n_refl n_p, n_a n_b or the number of workgroups (ceil(n_a / 8) ceil(n_b / 64) n_refl)
 *           beyond 2^31 - 1: -5; before any HIP call.  No workspace.  The _dev entry allocates nothing and does not synchronise
 *           (capturable); the host twin stages through the device's arena (one table uploaded when tt_b is NULL or tt_a, only
 *           the outputs asked for downloaded).
 * Kernel, resources and measured figures on MI355X: DESIGN.md section 4 (specular echoes of a sampled reflector).
 * ---------------------------------------------------------------------------------------- */
int rtus_specular_dev(const double *d_tt_a, int n_a, const double *d_tt_b, int n_b, int n_refl, int n_p,
                      double *d_t, double *d_pos, int *d_n_min, void *stream);
int rtus_specular(const double *tt_a, int n_a, const double *tt_b, int n_b, int n_refl, int n_p,
                  double *t, double *pos, int *n_min, int device);

/* ------------------------------------------------------------------------------------------
 * rtus_skip_reflector: skip legs off a sampled backwall.  A skip leg element e -> boundary point B -> focal point F is stationary
 * over B in t(e -> B) + |F - B| / c_up (Fermat).  t(e -> B) is any table of this library over the boundary's points — through
 * layers, a measured surface, the lens and pipe; the up leg is a straight segment in one medium.  This is rtus_specular's reduction
 * with focal points in the place of receivers and the up leg formed on the fly: the n_f x n_p table of up legs is never stored.
 * The Python layer builds on it the skip legs and the leg tables of multi-view TFM under a backwall of any sampled shape, under
 * layers and under a measured surface (api.skip_travel_time_reflector, skip_travel_time_layers_profile,
 * skip_travel_time_surface_profile, view_legs_layers_profile, view_legs_surface_profile, reflector_mask, backwall_profile).  NOT IN
 * THE REFERENCE; checked bit for bit against tests/skip_reflector_numpy.py and against rtus_specular.
 *   tt_down [n_e][n_p]  times from the n_e elements to the reflector's points, in order along the reflector — the shape any table
 *                       call over (xb, zb) returns
 *   xb, zb  [n_p]       the reflector's points;  c_up: the speed of the up leg;  xf, zf [n_f]: the focal points
 *   tt      [n_e][n_f]  the leg table, row-major like every other leg table;  pos [n_e][n_f] fp64, nullable: the bounce point in
 *                       units of the point index;  n_min [n_e][n_f] int32, nullable
 * Definition, for element e and focal point f:
 *   u_j: dx = xf - xb_j;  dz = zf - zb_j;  r2 = dx dx + dz dz;  d = sqrt(r2);  u_j = d / c_up — in exactly this order, each
 *           product and the sum rounded on their own (no fused multiply-add), the root and the division correctly rounded.  This is
 *           NumPy's np.sqrt(dx*dx + dz*dz) / c_up; it is not np.hypot.
 *   S_j = tt_down[e][j] + u_j, one fp64 addition.  S_j is FINITE when isfinite(S_j).  A coordinate that is not finite makes its
 *           S_j NaN or infinite, hence not finite: no special case.
 *   No S_j finite: tt = pos = NaN, n_min = 0.
 *   j* = the FIRST index attaining the least finite S_j.
 *   n_min = the number of j in [1, n_p - 2] with S_(j-1), S_j, S_(j+1) all finite, S_j < S_(j-1) and S_j < S_(j+1).  A diagnostic:
 *           above 1, two bounce points compete.
 *   j* = 0 or j* = n_p - 1, or a neighbour of j* not finite: tt = NaN, pos = (double) j* — the bounce point is not bracketed by the
 *           sampled span.
 *   Otherwise, with a = S_(j*-1), b = S_(j*), c = S_(j*+1), in exactly this order and every operation rounded on its own (no
 *           fused multiply-add; the division correctly rounded):
 *             d1 = a - c;  d2 = (a - b) + (c - b);  delta = 0.5 d1 / d2;  tt = b - (0.25 d1) delta;  pos = j* + delta.
 *   n_p < 3 is legal: every entry comes out NaN by the rules above.
 *   Consequence: tt, pos and n_min are bit-equal to rtus_specular(tt_down, n_e, U, n_f, 1, n_p, ...) with U[f][j] = u_j.
 *   Accuracy and sampling: the parabola's value error is third order in the point spacing in general; it is fourth order only where
 *           S is symmetric about its minimum, the case rtus_specular's section quotes.  The constant grows as the focal point nears
 *           the reflector.  One medium at 5900 m/s, 16 elements at 0.6 mm pitch on z = 0, a flat backwall at 30 mm sampled over
 *           +-20 mm, 17 x 21 points over x +-8 mm, z 6 - 26 mm, against the mirror image: 4.3e-10, 6.3e-11, 7.3e-12 s at 41, 81,
 *           161 points (1, 0.5, 0.25 mm); tilted by 5 degrees: 7.2e-10, 7.3e-11, 1.0e-11 s.  Sample the backwall at a quarter of a
 *           millimetre or finer for points a few millimetres off the wall.  A point whose bounce falls outside the sampled span is
 *           NaN, so the span must overhang the image.
 *   Not checked: the straight up leg against the polyline.  On a strongly re-entrant profile an up leg may cross the reflector; it
 *           is timed as if the boundary were not in its way.  Stationary maxima are not looked for.
 *   Determinism: an entry's bits depend only on its own row of tt_down, the reflector and its own focal point — not on the other
 *           entries of the call, nor on the launch shape, nor on which optional outputs are asked for.
 *   Limits: null tt_down, xb, zb, xf, zf or tt, a size <= 0, c_up not finite or not > 0: -1; n_e n_f or the number of workgroups
 *           (ceil(n_e / 8) ceil(n_f / 64)) beyond 2^31 - 1: -5; before any HIP call.  No workspace.  The _dev entry allocates
 *           nothing and does not synchronise (capturable); the host twin stages through the device's arena and downloads only the
 *           outputs asked for.
 * Kernel, resources and measured figures on MI355X: DESIGN.md section 4 (skip legs off a sampled backwall).
 * ---------------------------------------------------------------------------------------- */
int rtus_skip_reflector_dev(const double *d_tt_down, int n_e, const double *d_xb, const double *d_zb, int n_p, double c_up,
                            const double *d_xf, const double *d_zf, int n_f,
                            double *d_tt, double *d_pos, int *d_n_min, void *stream);
int rtus_skip_reflector(const double *tt_down, int n_e, const double *xb, const double *zb, int n_p, double c_up,
                        const double *xf, const double *zf, int n_f, double *tt, double *pos, int *n_min, int device);

/* ------------------------------------------------------------------------------------------
 * rtus_tfm_phase_hmc: rtus_tfm_phase over a HALF-MATRIX CAPTURE — rtus_tfm_analytic_hmc's delay-and-sum over the packed triangle
 * with the vector and sign coherence factors.  NOT IN THE REFERENCE; checked against tests/tfm_hmc_ext_numpy.py and against
 * rtus_tfm_phase on the unpacked capture.
 *   a [n_pairs][n_t][2], n_e, n_t, fs, t0, tt_tx, tt_rx [n_e][n_f] (the two may be one table), n_f: rtus_tfm_analytic_hmc's.
 *   The sample positions, the interpolation, the edge rules, the no-path rule, the pair rule and the order of summation are exactly
 *           rtus_tfm_analytic_hmc's (blocks of 16 columns; the rows above a block, then the block's triangle).
 *   image   [n_f][2]  BIT-IDENTICAL to rtus_tfm_analytic_hmc's image, whichever of the other outputs are asked for.
 *   Per record (i, j), i < j: the two samples p1 = a_ij(s_ij) and p2 = a_ij(s_ji); the diagonal has p1 = a_ii(s_ii) only.
 *   N = T R, rtus_tfm_analytic_hmc's count (R = T with one table).  As in rtus_tfm_phase a leg pair with a path whose position is
 *           outside the record counts in N with a zero phasor and a zero sign.
 *   U       accumulates u(p1) + u(p2) — the two of a pair added to each other FIRST, then to the running sum as one term; the
 *           diagonal u(p1) — in fp32 in the fixed order; u is rtus_tfm_phase's unit phasor (the same statements).
 *   One table (tt_tx == tt_rx as pointers): p1 == p2 bit for bit, so the record is gathered ONCE and U = fmaf(wgt, u(p1), U) with
 *           wgt = 2 off the diagonal, 1 on it: U + (u + u) in one rounding, the bits of the two-table form called with two equal
 *           tables.
 *   B       accumulates sign(Re p1) + sign(Re p2) (the diagonal sign(Re p1)) as an int32, exact; with one table the one sign is
 *           added twice off the diagonal.
 *   vcf, scf [n_f] float32, counts [n_f][2] int32 (B, N), all nullable: rtus_tfm_phase's formulas, clamps and NaN rule, formed in
 *           fp64 from the sums.  An output that is not asked for costs nothing in the gather loop.
 *   Consequence: counts and scf are BIT FOR BIT rtus_tfm_phase's on the unpacked capture (record (i, j) at [i][j] and [j][i]) with
 *           the same table(s), for any finite data: every pair's sample has the same bits in both forms — the same fp32 position,
 *           the same two loaded samples, the same fmaf — and B and N are integers, whose sums have no order.  vcf differs by the
 *           order of the fp32 sum of U alone.
 *   Determinism: the bits of a focal point depend only on its own columns of the tables; no output's bits depend on which other
 *           outputs are asked for.
 *   Limits: rtus_tfm_analytic_hmc's (image required; vcf, scf, counts nullable) and n_e^2 <= 2^30 (the sign sum is an int32; with
 *           n_e <= 32768 that is always so): -1 for invalid arguments, -5 past a limit, before any HIP call.  The _dev entry
 *           allocates nothing and does not synchronise (capturable).  The host twin stages through the arena (one table uploaded
 *           when tt_tx == tt_rx, only the outputs asked for downloaded).
 *
 * rtus_tfm_weighted_hmc: rtus_tfm_weighted over a half-matrix capture — ray-amplitude weighting and the sensitivity P, which put
 * the views of a multi-view inspection on one scale (|S| / P).  NOT IN THE REFERENCE; checked against tests/tfm_hmc_ext_numpy.py
 * and against rtus_tfm_weighted on the unpacked capture.
 *   a, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f: rtus_tfm_analytic_hmc's;  w_tx, w_rx [n_e][n_f][2] interleaved complex float32, both
 *           required (they may be one table);  image [n_f][2];  sens [n_f] float32, nullable.
 *   Legs:   element i's transmit leg has a path only if tt_tx[i] has one (rtus_tfm's rule) AND both parts of w_tx[i] are finite;
 *           its receive leg likewise from tt_rx[i] and w_rx[i].  A leg without a path contributes nothing and cannot poison the
 *           pixel: its weight counts as 0 (and, with two delay tables, its delay as the no-path value).
 *   Terms:  W_ij = w_tx[i] w_rx[j];  c_ii = W_ii a_ii(s_ii);  c_ij = W_ij a_ij(s_ij) + W_ji a_ij(s_ji) for i < j — the pair's two
 *           terms added to each other FIRST, then to the running sum.  S = the sum of the c in rtus_tfm_hmc's order (blocks of 16
 *           columns).  In exact arithmetic this is rtus_tfm_weighted on the symmetric full matrix.
 *   The fp32 statements (every product and sum rounded by itself but inside an fmaf; a = (ar, ai), b = (br, bi)):
 *             a b  :  re = fmaf(-ai, bi, ar br);   im = (ar bi) + (ai br)        — symmetric in a and b: a b == b a bit for bit,
 *                                                                                  so ONE weight table for both legs gives W_ij == W_ji
 *             W p  :  re = fmaf(-Wi, pi, Wr pr);   im = fmaf(Wr, pi, Wi pr)
 *           two delay tables:  c = (W_ij p1) + (W_ji p2), each part one addition;  S.re += c.re;  S.im += c.im
 *           one delay table (tt_tx == tt_rx as pointers; the weight tables may differ — every same-leg view "A-A", whose down and up
 *           amplitudes are different tables): s_ij == s_ji bit for bit, the record is gathered ONCE:
 *                              W = W_ij + W_ji, each part one addition (the diagonal: W = W_ii);  c = W p;  S += c as above.
 *   sens    P = (sum over the transmit legs with a path of |w_tx|^2) (sum over the receive legs with a path of |w_rx|^2): BIT FOR
 *           BIT rtus_tfm_weighted's sens on the same tables and weights — each sum the chain fmaf(wi, wi, fmaf(wr, wr, sum)) over
 *           the elements ascending, in fp32; the product in fp64, rounded once.  Passing sens does not change the bits of image.
 *   Determinism: the bits of a focal point depend only on its own columns of the tables and of the weights, and not on the size of
 *           the kernel's tile.
 *   Limits: rtus_tfm_analytic_hmc's; w_tx or w_rx null: -1.  The _dev entry allocates nothing and does not synchronise
 *           (capturable).  The host twin stages through the arena (one delay table and one weight table uploaded where the
 *           pointers are equal).
 * Measured on MI355X (2026-10-21; DESIGN.md §4 "Half-matrix capture", profiles/tfm_hmc_phase_weighted_kernel.txt; CUDA-event timing;
 * x = time / the full-matrix twin, rtus_tfm_phase_dev / rtus_tfm_weighted_dev on the unpacked capture with the same outputs, in the
 * SAME run; rtus_tfm_analytic_hmc_dev in that run: 143.8 us and 1.052 ms): 64 elements x 2048 samples, one delay table, 256^2 focal
 * points: phase image alone 143 us (0.53x), vcf 152 us (0.54x), scf 149 us (0.55x), all outputs 168 us (0.56x); weighted 233-235 us
 * (0.56x), with sens 237 us (0.61-0.62x); 1024^2: phase 1.03 / 1.43 / 1.12 / 1.61 ms (0.53-0.55x); weighted 1.89-1.99 ms
 * (0.62-0.68x).  Two delay tables: phase 0.75-1.10x; weighted 0.70-0.77x at 256^2 and 1.46-1.55x (slower than the twin) at 1024^2,
 * where one workgroup per CU (96 KiB of LDS) binds.  Not measured: counters, kernel durations under a profiler.
 * ---------------------------------------------------------------------------------------- */
int rtus_tfm_phase_hmc_dev(const float *d_a, int n_e, int n_t, double fs, double t0,
                           const double *d_tt_tx, const double *d_tt_rx, int n_f,
                           float *d_image, float *d_vcf, float *d_scf, int *d_counts, void *stream);
int rtus_tfm_phase_hmc(const float *a, int n_e, int n_t, double fs, double t0,
                       const double *tt_tx, const double *tt_rx, int n_f,
                       float *image, float *vcf, float *scf, int *counts, int device);
int rtus_tfm_weighted_hmc_dev(const float *d_a, int n_e, int n_t, double fs, double t0,
                              const double *d_tt_tx, const double *d_tt_rx, const float *d_w_tx, const float *d_w_rx, int n_f,
                              float *d_image, float *d_sens, void *stream);
int rtus_tfm_weighted_hmc(const float *a, int n_e, int n_t, double fs, double t0,
                          const double *tt_tx, const double *tt_rx, const float *w_tx, const float *w_rx, int n_f,
                          float *image, float *sens, int device);

/* ------------------------------------------------------------------------------------------
 * Matrix (2-D) arrays: element x focal-point Fermat travel times in THREE dimensions through horizontal layers — the table that
 * volumetric TFM needs.  NOT IN THE REFERENCE; checked against oracle/ per element, closed forms and tests/layers3d_numpy.py.
 * Every consumer of a table [n_e][n_f] (rtus_tfm*, rtus_focal_delays, rtus_fmc_sim, the multi-view entries) takes this one as it
 * is: the focal points are a flat list, the n_e = n_x n_y elements of a matrix array are rows.
 *
 *   z_if, c, n_if   the stack, rtus_tt_layers's conventions (HOST memory; n_if <= RTUS_MAX_LAYERS)
 *   xe,ye,ze [n_e]  elements, at any depth (also below the first interface)
 *   xf,yf,zf [n_f]  focal points, at any depth
 *   tt [n_e][n_f]   least travel time [s]; NaN where zf <= ze or where any of the pair's six coordinates is not finite
 *   flags           must be 0 (RTUS_ERR_INVALID_ARG otherwise): no tau-p tier, no table-served path
 *
 * Definition.  Horizontal layers are symmetric about the vertical axis: the ray from an element to a point lies in the vertical
 * plane through both, and its time is the planar time (rtus_tt_layers, default tier: <= 1e-13 relative) at the lateral reach
 *       r = sqrt(dx dx + dy dy),   dx = xf - xe,   dy = yf - ye
 * in fp64 with a correctly rounded square root, between the depths ze and zf.  With dy = 0, r is |dx| exactly.
 * Each entry depends on its own pair only.  Every solve starts from a bound formed from its own reach and depths; nothing is carried
 * from element to element.  The bits of tt[e][f] do not change when elements or points are permuted, duplicated, added or removed,
 * or when the call is split into calls over blocks of rows or columns.  Row shards and several GPUs therefore need no entry of
 * their own: a slice of the inputs gives the slice of the table.
 * Launch shape (what a test of the tile seams needs): one workgroup = RTUS_TT_LAYERS3_POINTS points (one per lane) x
 * RTUS_TT_LAYERS3_ROWS consecutive elements.
 * Limits: n_f < 2^29 (a row's byte offsets are 32-bit; row offsets are 64-bit, n_e n_f 8 may pass 4 GiB) and
 * ceil(n_f / RTUS_TT_LAYERS3_POINTS) ceil(n_e / RTUS_TT_LAYERS3_ROWS) < 2^31: RTUS_ERR_UNSUPPORTED beyond.  Null pointers, non-positive
 * sizes, a bad stack: as rtus_tt_layers.  The _dev entry allocates nothing and does not synchronise (capturable); the host twin stages
 * through the arena.
 * Measured on MI355X (2026-10-21; DESIGN.md section 4 "Matrix arrays", profiles/layers3d_kernel.txt; CUDA-event timing, two interfaces):
 * 16 x 16 elements x 64 x 64 x 32 points 152 us, 32 x 32 x 64^3 1.04 ms: 2.2-2.6e11 solves/s, 1.9-2.0x the time of rtus_tt_layers_dev
 * (default tier) at equal n_e and n_f in the same run — every solve starts cold.  Not measured: counters.
 * ---------------------------------------------------------------------------------------- */
#define RTUS_TT_LAYERS3_POINTS 256
#define RTUS_TT_LAYERS3_ROWS 16
int rtus_tt_layers3_dev(const double *z_if, const double *c, int n_if,
                        const double *d_xe, const double *d_ye, const double *d_ze, int n_e,
                        const double *d_xf, const double *d_yf, const double *d_zf, int n_f,
                        double *d_tt, unsigned flags, void *stream);
int rtus_tt_layers3(const double *z_if, const double *c, int n_if,
                    const double *xe, const double *ye, const double *ze, int n_e,
                    const double *xf, const double *yf, const double *zf, int n_f,
                    double *tt, unsigned flags, int device);

/* ------------------------------------------------------------------------------------------
 * Travel times into a homogeneous ANISOTROPIC part (austenitic weld metal, cladding, carbon-fibre laminate): the speed depends on
 * the ray's direction.  NOT IN THE REFERENCE — "parity unpinned"; checked against tests/aniso_numpy.py, with an isotropic series
 * against rtus_tt_surface, and with an elliptical one under a flat surface against rtus_tt_layers at stretched depths.
 *
 * The medium is its GROUP SLOWNESS over the ray's direction, a Fourier series of period pi:
 *
 *     S(psi) = a[0] + sum over k = 1 .. K of ( a[k] cos 2k psi + b[k] sin 2k psi ),    0 <= K <= 16,   b[0] is ignored
 *
 *   psi           the ray's angle from the +z axis (depth, down), positive towards +x: a leg from P to F has
 *                 psi = atan2(F_x - P_x, F_z - P_z); its sign is immaterial (the period).  The time along a straight leg of
 *                 length L is L S(psi).  K = 0, a[0] = 1 / c2 is the isotropic medium.
 *   a, b [K + 1]  HOST memory in both twins (passed to the kernels by value).  -1 (RTUS_ERR_INVALID_ARG) for K outside 0 .. 16,
 *                 for a coefficient that is not finite, and for a series that is not positive at one of the 4096 angles
 *                 psi_i = i pi / 4096.  The medium IS the series: how a series is fitted to a crystal's group slowness is the
 *                 host's business (the Python package: group_slowness_ti, fit_group_slowness, elliptical_slowness).
 *
 * rtus_tt_aniso_surface: through ONE measured surface, the couplant (c1) above it.  x0, dx, zs, n_s, c1, xe, ze, xf, zf, tt,
 *   x_entry, the workspace and the limits are rtus_tt_surface's, and so is the definition with the second leg changed:
 *
 *     T(x) = |E - S(x)| / c1 + |F - S(x)| S(psi(x)),    S(x) = (x, s(x)),  psi(x) the direction from S(x) to F
 *
 *   the entry is the LEAST T OVER THE INTERIOR LOCAL MINIMA of T; NaN without one, for an element with ze >= min s, for a focal
 *   point outside the extent or with zf <= s(xf), and for non-finite coordinates.  Occlusion is not checked.
 *   Guarantee: every interior local minimum whose basin spans at least one profile segment dx centred on it is found — the basin
 *   running from the minimum to its neighbouring stationary points of T or to the ends of the extent; a minimum qualifies when
 *   each neighbouring STATIONARY point is at least dx / 2 away (an end of the extent always does).  Narrower minima may be
 *   missed; a missed minimum can only make the reported time later (or NaN), never earlier.  The entry is the least T over the
 *   found minima where there are at most three of them.  With four or more, the three are chosen by a lower bound of each one's T
 *   taken at a scan point next to it (spacing dx / 4: within T'' (dx / 4)^2 of the minimum's own T, ~2e-8 s on a 1 mm grid); the
 *   least minimum can be left out where it is within that of the third chosen one, and the entry is then late by at most that much.
 *   Determinism: an entry depends only on its element, its focal point, the profile, c1 and the coefficients — not on which other
 *   elements or focal points share the call (the bits of a row block or a focal-point subset are those of the whole table).
 *   The _dev entry runs rtus_tt_surface's set-up kernel (into d_workspace: rtus_tt_surface_workspace_bytes(n_s) bytes, 256-byte
 *   aligned, -4 otherwise) and the table kernel on `stream`: no allocation, no host synchronisation (capturable).
 *
 * rtus_tt_aniso_direct: CONTACT, the probe on the part and no couplant path: the ray is straight, tt[e][f] = |F - E| S(psi), psi
 *   the direction from E to F.  Any relative position is accepted (a point above the element: the period); 0 at zero distance;
 *   NaN for a non-finite coordinate.  n_e <= 65535 (-5 beyond).  Each entry depends on its own pair and the coefficients only.
 * ---------------------------------------------------------------------------------------- */
int rtus_tt_aniso_surface_dev(double x0, double dx, const double *d_zs, int n_s, double c1,
                              const double *a, const double *b, int K,
                              const double *d_xe, const double *d_ze, int n_e,
                              const double *d_xf, const double *d_zf, int n_f,
                              double *d_tt, double *d_x_entry, void *d_workspace, size_t workspace_bytes, void *stream);
int rtus_tt_aniso_surface(double x0, double dx, const double *zs, int n_s, double c1,
                          const double *a, const double *b, int K,
                          const double *xe, const double *ze, int n_e,
                          const double *xf, const double *zf, int n_f,
                          double *tt, double *x_entry, int device);
int rtus_tt_aniso_direct_dev(const double *a, const double *b, int K,
                             const double *d_xe, const double *d_ze, int n_e,
                             const double *d_xf, const double *d_zf, int n_f, double *d_tt, void *stream);
int rtus_tt_aniso_direct(const double *a, const double *b, int K,
                         const double *xe, const double *ze, int n_e,
                         const double *xf, const double *zf, int n_f, double *tt, int device);

#ifdef __cplusplus
}
#endif
#endif /* RTUS_H */
