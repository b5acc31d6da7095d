// rtus_capi.hip — the extern "C" boundary declared in include/rtus.h.
// *_dev: device pointers + stream, asynchronous, no allocation.  Host twins: stage through HBM.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <dlfcn.h>
#include <mutex>
#include <numeric>
#include <string.h>
#include <thread>
#include <vector>
#include "../../include/rtus.h"

// launchers (rtus_shoot.hip / rtus_match.hip / rtus_fermat.hip)
size_t rtus_ws_bytes(int n);
hipError_t rtus_selftest_run(const rtus_lens& lens, int n, long long n_math, unsigned long long counts[4], hipStream_t s);
hipError_t rtus_launch_shoot(const rtus_lens& lens, const double* geoms, int n_geom, const double* x_a,
                             const double* z_a, int n_tx, const double* alpha, const double* z_f, int n,
                             double* out8, double* tof4, double* tof, double* land_x, uint8_t* status,
                             void* ws, unsigned flags, hipStream_t s);
size_t rtus_solve_ws_bytes(int n, int n_geom, int n_tx, int n_rx);
hipError_t rtus_launch_solve(const rtus_lens& lens, const double* geoms, int n_geom, const double* x_a,
                             const double* z_a, int n_tx, const double* alpha, int n, const double* x_rx, int n_rx,
                             double z_land, double* tt, double* alpha_root, double* tt_all,
                             double* alpha_all, uint8_t* n_roots, void* ws, unsigned flags, hipStream_t s);
size_t rtus_sweep_ws_bytes(int n, int n_geom, int n_tx, int n_rx);
hipError_t rtus_launch_sweep(const rtus_lens& lens, const double* geoms, int n_geom, const double* x_a, const double* z_a, int n_tx,
                             const double* alpha, const double* z_f, int n, const double* x_rx, int n_rx, double atol, double rtol,
                             int32_t* first_ray, uint8_t* hit, double* tof_hit, double* tof, double* land_x, void* ws, unsigned flags,
                             hipStream_t s);
hipError_t rtus_launch_match(const double* land_x, const double* tof, int n_batch, int n, const double* x_rx,
                             int n_rx, double atol, double rtol, int32_t* first_ray,
                             uint8_t* hit, double* tof_hit, uint8_t* ray_hit, hipStream_t s);
hipError_t rtus_launch_tt_layers(const double* z_if, const double* c, int n_if, const double* xe,
                                 const double* ze, int n_e, const double* xf, const double* zf, int n_f,
                                 double* tt, uint8_t* iters, unsigned flags, hipStream_t s);
hipError_t rtus_launch_tt_layers_batch(const double* z_if, const double* c, int n_if, const double* xe, const double* ze,
                                       int n_e, long long e_stride, const double* xf, const double* zf, int n_f,
                                       long long f_stride, double* tt, long long t_stride, int n_batch, unsigned flags, hipStream_t s);
hipError_t rtus_launch_tt_layers_rows(const double* z_if, const double* c, int n_if, const double* xe, const double* ze, int n_e,
                                      int row0, long long n_rows_total, const double* xf, const double* zf, int n_f, double* tt,
                                      unsigned flags, hipStream_t s);
int rtus_rows_per_block(long long n_rows_total, int n_f, int n_batch, int elem_bytes);
size_t rtus_layers_sort_ws_bytes(int n_e);
hipError_t rtus_launch_tt_layers_sorted(const double* z_if, const double* c, int n_if, const double* xe, const double* ze, int n_e,
                                        const double* xf, const double* zf, int n_f, double* tt, void* ws, const int* presorted_row_of,
                                        unsigned flags, hipStream_t s);
hipError_t rtus_launch_tt_layers3(const double* z_if, const double* c, int n_if, const double* xe, const double* ye, const double* ze,
                                  int n_e, const double* xf, const double* yf, const double* zf, int n_f, double* tt, hipStream_t s);

hipError_t rtus_launch_tt_lens_f64(const rtus_lens& L, double a_lo, double a_hi, const double* xe, const double* ze,
                                   int n_e, const double* xf, const double* zf, int n_f, double* tt,
                                   double* alpha_out, int row0, long long n_rows_total, hipStream_t s, unsigned long long* stats = nullptr);
hipError_t rtus_launch_tt_lens_f32(const rtus_lens& L, double a_lo, double a_hi, const float* xe, const float* ze,
                                   int n_e, const float* xf, const float* zf, int n_f, float* tt, float* alpha_out,
                                   int row0, long long n_rows_total, hipStream_t s, unsigned long long* stats = nullptr);

hipError_t rtus_launch_tt_surface(double x0, double dx, const double* zs, int n_s, double c1, double c2, const double* xe,
                                  const double* ze, int n_e, const double* xf, const double* zf, int n_f, double* tt, double* xent,
                                  void* ws, hipStream_t s);
size_t rtus_surface_ws_bytes(int n_s);
hipError_t rtus_launch_tt_surface_skip(double x0, double dx, const double* zs, int n_s, double c1, double c_down, double c_up, double z_back,
                                       const double* xe, const double* ze, int n_e, const double* xf, const double* zf, int n_f, double* tt,
                                       double* xent, double* xback, void* ws, hipStream_t s);
hipError_t rtus_launch_tt_aniso_surface(double x0, double dx, const double* zs, int n_s, double c1, const double* a, const double* b, int K,
                                        const double* xe, const double* ze, int n_e, const double* xf, const double* zf, int n_f,
                                        double* tt, double* xent, void* ws, hipStream_t s);
hipError_t rtus_launch_tt_aniso_direct(const double* a, const double* b, int K, const double* xe, const double* ze, int n_e,
                                       const double* xf, const double* zf, int n_f, double* tt, hipStream_t s);
bool rtus_aniso_series_ok(const double* a, const double* b, int K);
hipError_t rtus_launch_focal_delays(const double* tt, int n_e, int n_f, double* delays, hipStream_t s);
hipError_t rtus_launch_tfm(const float* fmc, int n_tx, int n_rx, int n_t, double fs, double t0, const double* tt_tx,
                           const double* tt_rx, int n_f, float* image, hipStream_t s);
hipError_t rtus_launch_fmc_analytic(const float* fmc, long long n_pairs, int n_t, int n_taps, float2* out, hipStream_t s);
hipError_t rtus_launch_surface_find(const float* an, int n_e, int n_t, double fs, double t0, const double* xe, const double* ze,
                                    double c1, double x0, double dx, int n_s, double z_lo, double dz, int n_z, double* z_peak,
                                    float* amp, float* image, hipStream_t s);
hipError_t rtus_launch_echo_pick(const float* an, long long n_pairs, int n_t, double fs, double t0, double t_lo, double t_hi,
                                 const double* g_lo, const double* g_hi, double* t_pick, float* amp, hipStream_t s);
hipError_t rtus_launch_geom_misfit(const double* tt, int n_geom, int n_tx, int n_rx, const double* t_meas, const double* w, int* n,
                                   double* sse, double* sum_r, double* sum_w, hipStream_t s);
hipError_t rtus_launch_specular(const double* tt_a, int n_a, const double* tt_b, int n_b, int n_refl, int n_p, double* t, double* pos,
                                int* n_min, hipStream_t s);
long long rtus_specular_blocks(int n_a, int n_b, int n_refl);
hipError_t rtus_launch_skip_reflector(const double* tt_down, int n_e, const double* xb, const double* zb, int n_p, double c_up,
                                      const double* xf, const double* zf, int n_f, double* tt, double* pos, int* n_min, hipStream_t s);
long long rtus_skip_reflector_blocks(int n_e, int n_f);
hipError_t rtus_launch_tfm_analytic(const float* an, int n_tx, int n_rx, int n_t, double fs, double t0, const double* tt_tx,
                                    const double* tt_rx, int n_f, float* image, float* cf, hipStream_t s);
hipError_t rtus_launch_tfm_hmc(const float* hmc, int n_e, int n_t, double fs, double t0, const double* tt_tx, const double* tt_rx,
                               int n_f, float* image, hipStream_t s);
hipError_t rtus_launch_tfm_analytic_hmc(const float* an, int n_e, int n_t, double fs, double t0, const double* tt_tx,
                                        const double* tt_rx, int n_f, float* image, float* cf, hipStream_t s);
hipError_t rtus_launch_tfm_iq(const float* an, int n_tx, int n_rx, int n_t, double fs, double t0, double f_demod, const double* tt_tx,
                              const double* tt_rx, int n_f, float* image, float* cf, hipStream_t s);
hipError_t rtus_launch_tfm_iq_hmc(const float* an, int n_e, int n_t, double fs, double t0, double f_demod, const double* tt_tx,
                                  const double* tt_rx, int n_f, float* image, float* cf, hipStream_t s);
hipError_t rtus_launch_fmc_pack_frames(const float* stack, int n_frames, size_t n, float* packed, hipStream_t s);
hipError_t rtus_launch_tfm_frames(const float* packed, int n_frames, int n_tx, int n_rx, int n_t, double fs, double t0,
                                  const double* tt_tx, const double* tt_rx, int n_f, float* images, hipStream_t s);
hipError_t rtus_launch_tfm_analytic_frames(const float* an, int n_frames, int n_tx, int n_rx, int n_t, double fs, double t0, double f_demod,
                                           const double* tt_tx, const double* tt_rx, int n_f, float* images, float* cf, hipStream_t s);
long long rtus_tfm_frames_blocks(int n_slow, int n_f);
hipError_t rtus_launch_fmc_pack_frames_i16(const short* stack, int n_frames, size_t n, short* packed, hipStream_t s);
hipError_t rtus_launch_tfm_frames_i16(const short* packed, int n_frames, int n_tx, int n_rx, int n_t, double fs, double t0,
                                      const double* tt_tx, const double* tt_rx, int n_f, float* images, hipStream_t s);
hipError_t rtus_launch_tfm_frames_hmc_i16(const short* packed, int n_frames, int n_e, int n_t, double fs, double t0, const double* tt_tx,
                                          const double* tt_rx, int n_f, float* images, hipStream_t s);
hipError_t rtus_launch_tfm_frames_hmc(const float* packed, int n_frames, int n_e, int n_t, double fs, double t0, const double* tt_tx,
                                      const double* tt_rx, int n_f, float* images, hipStream_t s);
hipError_t rtus_launch_fmc_analytic_i16(const short* stack, int n_frames, long long n_scans, int n_t, int n_taps, bool pairs, float* out,
                                        hipStream_t s);
hipError_t rtus_launch_envelope_combine(const float* re, const float* im, size_t n, bool mag, float* out, hipStream_t s);
hipError_t rtus_launch_tfm_weighted(const float* an, int n_tx, int n_rx, int n_t, double fs, double t0, const double* tt_tx,
                                    const double* tt_rx, const float* w_tx, const float* w_rx, int n_f, float* image, float* sens,
                                    hipStream_t s);
hipError_t rtus_launch_tfm_phase(const float* an, int n_tx, int n_rx, int n_t, double fs, double t0, const double* tt_tx,
                                 const double* tt_rx, int n_f, float* image, float* vcf, float* scf, int* counts, hipStream_t s);
hipError_t rtus_launch_tfm_phase_hmc(const float* an, int n_e, int n_t, double fs, double t0, const double* tt_tx, const double* tt_rx,
                                     int n_f, float* image, float* vcf, float* scf, int* counts, hipStream_t s);
hipError_t rtus_launch_tfm_weighted_hmc(const float* an, int n_e, int n_t, double fs, double t0, const double* tt_tx, const double* tt_rx,
                                        const float* w_tx, const float* w_rx, int n_f, float* image, float* sens, hipStream_t s);
hipError_t rtus_launch_leg_amp_surface(double x0, double dx, const double* zs, int n_s, double c1, double rho1, double c_l, double c_t,
                                       double rho2, double z_back, int leg, int up, double width, double f_c, const double* xe,
                                       const double* ze, int n_e, const double* xf, const double* zf, int n_f, const double* x_entry,
                                       const double* x_back, float* amp, void* ws, hipStream_t s);
hipError_t rtus_launch_pw_layers(const double* z_if, const double* c, int n_if, const double* ang, int n_a, double xlo, double xhi,
                                 double za, const double* xf, const double* zf, int n_f, double* tt, hipStream_t s);
hipError_t rtus_launch_pw_surface(double x0, double dx, const double* zs, int n_s, double c1, double c2, const double* ang, int n_a,
                                  double xlo, double xhi, double za, const double* xf, const double* zf, int n_f, double* tt, double* xent,
                                  void* ws, hipStream_t s);
hipError_t rtus_launch_tt_pipe(const rtus_lens& L, double a_lo, double a_hi, const rtus_pipe& P, double b_lo, double b_hi, int n_scan,
                               const double* xe, const double* ze, int n_e, const double* xf, const double* zf, int n_f, double* tt,
                               double* alpha_out, double* beta_out, void* ws, hipStream_t s);
size_t rtus_pipe_ws_bytes(int n_e, int m);
hipError_t rtus_launch_tt_pipe_skip(const rtus_lens& L, double a_lo, double a_hi, const rtus_pipe& P, double c_up, double b_lo, double b_hi,
                                    int n_scan, const double* xe, const double* ze, int n_e, const double* xf, const double* zf, int n_f,
                                    double* tt, double* alpha_out, double* beta_out, double* gamma_out, void* ws, hipStream_t s);
hipError_t rtus_launch_leg_amp_pipe(const rtus_lens& L, double a_lo, double a_hi, const rtus_pipe& P, const rtus_pipe_media& M, int leg,
                                    int up, double width, double f_c, const double* xe, const double* ze, int n_e, const double* xf,
                                    const double* zf, int n_f, const double* alpha, const double* beta, const double* gamma, float* amp,
                                    hipStream_t s);
hipError_t rtus_launch_fmc_synth_tx(const float* fmc, int n_tx, int n_rx, int n_t, double fs, const double* d, int n_v, float* out,
                                    hipStream_t s);
hipError_t rtus_launch_fmc_sim(const double* t1, const double* t2, const float* q, const float* a1, const float* a2, int n_tx, int n_rx,
                               int n, int echo, const float* pulse, int n_p, int centre, int os, double fs, double t0, int n_t, float* out,
                               int analytic, int accumulate, hipStream_t s);

static thread_local int g_last_hip = 0;
static int hip_fail(hipError_t e) { g_last_hip = (int)e; return RTUS_ERR_HIP; }
#define HIP_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return hip_fail(e_); } while (0)
// a launcher reports hipGetLastError(): clear it first, so that a stale error of an unrelated earlier HIP call (the
// caller's, torch's) is not taken for this launch's
#define LAUNCH_TRY(x) do { (void)hipGetLastError(); HIP_TRY(x); } while (0)

// ---------------------------------------------------------------------------------------------------------
// Host-buffer twins: staging through a per-device arena.  The reference's calling pattern is hundreds of small
// sequential calls (main_rt.py:464-482: 210 x shoot_rays(N = 905)); a hipMalloc / hipFree pair per buffer and call
// (up to 11 of them) plus the null stream's implicit synchronisation cost more than the kernels.  So: one grow-only
// device allocation and one non-blocking stream per device, created on first use and kept until rtus_release(); a call
// locks its device's arena for its duration (host-buffer calls on ONE device are serialised; the *_dev entry points
// are untouched: caller's pointers, caller's stream, no state).
// ---------------------------------------------------------------------------------------------------------
namespace {
constexpr int kMaxDevices = 64;
constexpr int kMaxSlots = 4;                        // arenas per device: a multi-device call may list a device more than once
constexpr size_t kPinBytes = (size_t)1 << 20;       // per direction: calls that move less than this go through ONE copy
struct Arena {
    std::mutex mu;
    void* dev = nullptr;
    size_t cap = 0;
    char* pin = nullptr;                            // 2 x kPinBytes of page-locked host memory: [0, k) up, [k, 2k) down
    hipStream_t stream = nullptr;
    // rtus_shoot's lens polyline, kept between calls: the reference's script calls shoot_rays 210 times over ONE launch-angle
    // grid (main_rt.py:464-482), and the polyline launch is 9 of such a call's 43 us.  Valid for exactly the alpha values and
    // lens constants it was built from (compared byte for byte on every call).
    void* poly_ws = nullptr;
    size_t poly_cap = 0;
    std::vector<double> poly_alpha;
    rtus_lens poly_lens = {};
    bool poly_valid = false;
};
Arena g_arena[kMaxDevices][kMaxSlots];

// The twins run on `device` and put the caller's current device back when they return.
struct DeviceGuard {
    int prev = -1;
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// One host-buffer call on one device.  open() locks the device's arena; the twin then states each buffer once — in() an
// input, out() a result, scratch() device-only memory — and flush() lays them out, grows the arena to fit, binds the twin's
// pointers and copies the inputs; finish() copies every result back.  Nothing is placed before flush(): a declared pointer
// is nullptr until then (and stays nullptr for a count of 0 or an out() the caller does not want).
struct Session {
    enum Kind { kIn, kOut, kScratch };
    struct Buf { void** bind; void* host; size_t bytes, off; Kind kind; bool pinned; };
    static constexpr int kMaxBufs = 16;
    // (direct results: at most kPinBytes / 4 of data plus the alignment of each, inside the download half)
    static_assert(kPinBytes / 4 + kMaxBufs * 256 <= kPinBytes, "direct results must fit the page-locked buffer");
    static size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

    DeviceGuard guard;                 // (declared first: restored last, after the lock is gone)
    std::unique_lock<std::mutex> lock;
    Arena* a = nullptr;
    Buf buf[kMaxBufs];
    int n_buf = 0;
    bool overflow = false;             // more than kMaxBufs declared: flush() refuses the call
    // Small results written by the kernel STRAIGHT into the page-locked buffer (it is device-visible): no device-to-host copy
    // command behind the kernel (9 of a 32-us call) — the stores cross PCIe while the kernel runs.  (The same for the inputs —
    // the kernel reading them from the page-locked buffer instead of one small host-to-device copy — was measured: no gain.)
    // Opt-in per twin, before flush(); taken when all the results the call asks for are small.
    bool allow_direct = false;
    bool direct = false;

    int dev_index = -1;
    // the session ends with its stream drained whatever happened in between (an early return after flush() must not leave
    // copies in flight while the next call re-uses the page-locked buffer)
    bool drained = false;              // copy_back() came back clean: nothing in flight
    ~Session() { if (a && a->stream && !drained) (void)hipStreamSynchronize(a->stream); }
    int open(int device, int slot = 0)
    {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return RTUS_ERR_NO_DEVICE;
        if (device < 0 || device >= n || device >= kMaxDevices || slot < 0 || slot >= kMaxSlots) return RTUS_ERR_NO_DEVICE;
        dev_index = device;
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != device) guard.prev = cur;
        HIP_TRY(hipSetDevice(device));
        Arena* ar = &g_arena[device][slot];
        lock = std::unique_lock<std::mutex>(ar->mu);
        a = ar;
        if (!a->stream) HIP_TRY(hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking));
        if (!a->pin) HIP_TRY(hipHostMalloc((void**)&a->pin, 2 * kPinBytes, hipHostMallocDefault));
        return RTUS_OK;
    }
    void add(void** bind, void* host, size_t bytes, Kind kind)
    {
        *bind = nullptr;
        if (!bytes || (kind == kOut && !host)) return;
        if (n_buf == kMaxBufs) { overflow = true; return; }
        buf[n_buf++] = {bind, host, bytes, 0, kind, false};
    }
    template <class T> void in(T*& d, const T* h, size_t count) { add((void**)&d, (void*)h, count * sizeof(T), kIn); }
    template <class T> void out(T*& d, T* h, size_t count) { add((void**)&d, (void*)h, count * sizeof(T), kOut); }
    template <class T> void scratch(T*& d, size_t count) { add((void**)&d, nullptr, count * sizeof(T), kScratch); }
    // The inputs first, in declaration order, next to each other at the start of the arena; then the results and the scratch
    // in declaration order.  All inputs go in one host-to-device copy through the page-locked buffer when they are small (the
    // reference's calls are: 15 KB in, 58 KB out), one copy each otherwise.
    int flush()
    {
        if (overflow) return RTUS_ERR_UNSUPPORTED;
        size_t out_bytes = 0;
        for (int i = 0; i < n_buf; ++i) out_bytes += buf[i].kind == kOut ? buf[i].bytes : 0;
        direct = allow_direct && out_bytes + 8 * 256 <= kPinBytes / 4;
        size_t dev_bytes = 0, pin_bytes = 0, in_end = 0;
        for (bool inputs : {true, false})
            for (int i = 0; i < n_buf; ++i) {
                Buf& b = buf[i];
                if ((b.kind == kIn) != inputs) continue;
                b.pinned = direct && b.kind == kOut;
                size_t& end = b.pinned ? pin_bytes : dev_bytes;
                b.off = end;
                end += al256(b.bytes);
                if (inputs) in_end = b.off + b.bytes;
            }
        if (a->cap < dev_bytes) {                                    // grow-only; the previous call has synchronised
            if (a->dev) { (void)hipFree(a->dev); a->dev = nullptr; a->cap = 0; }
            const size_t want = (dev_bytes + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
            HIP_TRY(hipMalloc(&a->dev, want));
            a->cap = want;
        }
        for (int i = 0; i < n_buf; ++i) *buf[i].bind = (buf[i].pinned ? a->pin + kPinBytes : (char*)a->dev) + buf[i].off;
        const bool packed = in_end <= kPinBytes;
        for (int i = 0; i < n_buf; ++i) {
            if (buf[i].kind != kIn) continue;
            if (packed) memcpy(a->pin + buf[i].off, buf[i].host, buf[i].bytes);
            else HIP_TRY(hipMemcpyAsync((char*)a->dev + buf[i].off, buf[i].host, buf[i].bytes, hipMemcpyHostToDevice, a->stream));
        }
        if (packed && in_end) HIP_TRY(hipMemcpyAsync(a->dev, a->pin, in_end, hipMemcpyHostToDevice, a->stream));
        return RTUS_OK;
    }
    // after flush(): one more result, read back from a buffer declared as something else (a twin that works in place)
    template <class T> void download(T* h, const T* d, size_t count)
    {
        if (!h || !count) return;
        if (n_buf == kMaxBufs) { overflow = true; return; }
        buf[n_buf++] = {nullptr, (void*)h, count * sizeof(T), (size_t)((const char*)d - (const char*)a->dev), kOut, false};
    }
    int finish()
    {
        if (overflow) return RTUS_ERR_UNSUPPORTED;
        const hipError_t e = copy_back();
        return e == hipSuccess ? RTUS_OK : hip_fail(e);
    }
    // results back + synchronise: one device-to-host copy through the page-locked buffer when they are small.  (The HIP error
    // itself: table_multi runs it on a thread per device, and the last error is recorded per thread.)
    hipError_t copy_back()
    {
        char* stage = a->pin + kPinBytes;
        auto back = [](const Buf& b) { return b.kind == kOut && !b.pinned; };   // a result to copy back from the arena
        int n_back = 0;
        size_t lo = SIZE_MAX, hi = 0;
        for (int i = 0; i < n_buf; ++i)
            if (back(buf[i])) {
                ++n_back;
                lo = std::min(lo, buf[i].off);
                hi = std::max(hi, buf[i].off + buf[i].bytes);
            }
        if (direct) {                                                // results are in the page-locked buffer once the stream has drained
            const hipError_t e = hipStreamSynchronize(a->stream);
            if (e != hipSuccess) return e;
            drained = true;
            for (int i = 0; i < n_buf; ++i) if (buf[i].pinned) memcpy(buf[i].host, stage + buf[i].off, buf[i].bytes);
            if (!n_back) return hipSuccess;
        }
        if (n_back && hi - lo <= kPinBytes) {
            hipError_t e = hipMemcpyAsync(stage, (char*)a->dev + lo, hi - lo, hipMemcpyDeviceToHost, a->stream);
            if (e != hipSuccess) return e;
            e = hipStreamSynchronize(a->stream);
            if (e != hipSuccess) return e;
            drained = true;
            for (int i = 0; i < n_buf; ++i) if (back(buf[i])) memcpy(buf[i].host, stage + (buf[i].off - lo), buf[i].bytes);
            return hipSuccess;
        }
        for (int i = 0; i < n_buf; ++i) {
            if (!back(buf[i])) continue;
            const hipError_t e = hipMemcpyAsync(buf[i].host, (char*)a->dev + buf[i].off, buf[i].bytes, hipMemcpyDeviceToHost, a->stream);
            if (e != hipSuccess) return e;
        }
        const hipError_t e = hipStreamSynchronize(a->stream);
        drained = e == hipSuccess;
        return e;
    }
};

// *_dev entries: the caller's workspace is present, aligned to `align` bytes and large enough
int check_workspace(const void* ws, size_t bytes, size_t need, uintptr_t align)
{
    return ws && !((uintptr_t)ws & (align - 1)) && bytes >= need ? RTUS_OK : RTUS_ERR_WORKSPACE;
}
}   // namespace

// curved-lens helpers (C++ linkage: templates)
static int check_lens(const rtus_lens* lens, double a_lo, double a_hi, const void* xe, const void* ze, int n_e,
                      const void* xf, const void* zf, int n_f, const void* tt)
{
    if (!lens || !xe || !ze || !xf || !zf || !tt || n_e <= 0 || n_f <= 0) return RTUS_ERR_INVALID_ARG;
    if (n_e > 65535 * 64) return RTUS_ERR_UNSUPPORTED;
    if (!(a_hi > a_lo) || !isfinite(a_lo) || !isfinite(a_hi)) return RTUS_ERR_INVALID_ARG;
    if (!(lens->c1 > 0) || !(lens->c2 > 0) || lens->c1 == lens->c2) return RTUS_ERR_INVALID_ARG;
    return RTUS_OK;
}

template <typename R, typename F>
static int lens_host(const rtus_lens* lens, double a_lo, double a_hi, const R* xe, const R* ze, int n_e, const R* xf,
                     const R* zf, int n_f, R* tt, R* alpha_out, int device, F launch)
{
    int st = check_lens(lens, a_lo, a_hi, xe, ze, n_e, xf, zf, n_f, tt);
    if (st) return st;
    const size_t tot = (size_t)n_e * n_f;
    Session S;
    if ((st = S.open(device))) return st;
    R *dxe, *dze, *dxf, *dzf, *dtt, *dal;
    S.in(dxe, xe, n_e);
    S.in(dze, ze, n_e);
    S.in(dxf, xf, n_f);
    S.in(dzf, zf, n_f);
    S.out(dtt, tt, tot);
    S.out(dal, alpha_out, tot);
    if ((st = S.flush())) return st;
    LAUNCH_TRY(launch(*lens, a_lo, a_hi, dxe, dze, n_e, dxf, dzf, n_f, dtt, dal, 0, n_e, S.a->stream, nullptr));
    return S.finish();
}

extern "C" {

const char* rtus_strerror(int status)
{
    switch (status) {
        case RTUS_OK: return "ok";
        case RTUS_ERR_INVALID_ARG: return "invalid argument";
        case RTUS_ERR_NO_DEVICE: return "no usable HIP device";
        case RTUS_ERR_HIP: return "HIP runtime error (see rtus_last_hip_error)";
        case RTUS_ERR_WORKSPACE: return "workspace null or too small";
        case RTUS_ERR_UNSUPPORTED: return "unsupported size";
        default: return "unknown status";
    }
}
int rtus_version(void) { return RTUS_VERSION; }
int rtus_last_hip_error(void) { return g_last_hip; }
int rtus_release(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return RTUS_ERR_NO_DEVICE;
    if (device >= n || device >= kMaxDevices) return RTUS_ERR_NO_DEVICE;
    DeviceGuard guard;
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess) guard.prev = cur;
    for (int d = (device < 0 ? 0 : device); d < (device < 0 ? (n < kMaxDevices ? n : kMaxDevices) : device + 1); ++d) {
        for (int sl = 0; sl < kMaxSlots; ++sl) {
            Arena& a = g_arena[d][sl];
            std::lock_guard<std::mutex> lk(a.mu);
            if (!a.dev && !a.stream && !a.pin && !a.poly_ws) continue;
            HIP_TRY(hipSetDevice(d));
            if (a.stream) { (void)hipStreamSynchronize(a.stream); (void)hipStreamDestroy(a.stream); a.stream = nullptr; }
            if (a.dev) { (void)hipFree(a.dev); a.dev = nullptr; a.cap = 0; }
            if (a.poly_ws) { (void)hipFree(a.poly_ws); a.poly_ws = nullptr; a.poly_cap = 0; }
            a.poly_valid = false; a.poly_alpha.clear(); a.poly_alpha.shrink_to_fit();
            if (a.pin) { (void)hipHostFree(a.pin); a.pin = nullptr; }
        }
    }
    return RTUS_OK;
}

int rtus_device_count(int* count)
{
    if (!count) return RTUS_ERR_INVALID_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { *count = 0; return RTUS_ERR_NO_DEVICE; }
    *count = n;
    return RTUS_OK;
}

int rtus_selftest(const rtus_lens* lens, int n_rays, long long n_math, unsigned long long* counts, int device)
{
    if (!lens || !counts || n_rays < 8 || n_math < 0 || n_math > (1ll << 36)) return RTUS_ERR_INVALID_ARG;
    Session S;                                       // validates `device`, restores the caller's device, the arena's own stream
    int st = S.open(device);
    if (st) return st;
    LAUNCH_TRY(rtus_selftest_run(*lens, n_rays, n_math, counts, S.a->stream));
    return RTUS_OK;
}

// ---------------------------------------------------------------------------- forward trace
size_t rtus_shoot_workspace_bytes(int n_rays) { return n_rays > 0 ? rtus_ws_bytes(n_rays) : 0; }

static int check_shoot(const rtus_lens* lens, const void* geoms, int n_geom, const void* x_a, const void* z_a,
                       int n_tx, const void* alpha, const void* z_f, int n_rays)
{
    if (!lens || !geoms || !x_a || !z_a || !alpha || !z_f) return RTUS_ERR_INVALID_ARG;
    if (n_geom <= 0 || n_tx <= 0 || n_rays < 2) return RTUS_ERR_INVALID_ARG;   // curve needs >= 2 points (main_rt.py:26-27)
    if (n_geom > 65535 || n_tx > 65535) return RTUS_ERR_UNSUPPORTED;
    if (!(lens->c1 > 0) || !(lens->c2 > 0) || lens->c1 == lens->c2) return RTUS_ERR_INVALID_ARG;
    return RTUS_OK;
}
#define RTUS_SHOOT_KNOWN_FLAGS (RTUS_SHOOT_FAST_MATH | RTUS_TRUE_PIPE_TANGENT | RTUS_ANALYTIC_LENS | RTUS_POLYLINE_READY)

int rtus_shoot_dev(const rtus_lens* lens, const double* d_geoms, int n_geom, const double* d_x_a,
                   const double* d_z_a, int n_tx, const double* d_alpha, const double* d_z_f, int n_rays,
                   double* d_out8, double* d_tof4, double* d_tof, double* d_land_x, uint8_t* d_status,
                   void* d_workspace, size_t workspace_bytes, unsigned flags, void* stream)
{
    int st = check_shoot(lens, d_geoms, n_geom, d_x_a, d_z_a, n_tx, d_alpha, d_z_f, n_rays);
    if (st) return st;
    if (flags & ~RTUS_SHOOT_KNOWN_FLAGS) return RTUS_ERR_INVALID_ARG;
    if ((st = check_workspace(d_workspace, workspace_bytes, rtus_ws_bytes(n_rays), 64))) return st;
    LAUNCH_TRY(rtus_launch_shoot(*lens, d_geoms, n_geom, d_x_a, d_z_a, n_tx, d_alpha, d_z_f, n_rays, d_out8,
                              d_tof4, d_tof, d_land_x, d_status, d_workspace, flags, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_shoot(const rtus_lens* lens, const double* geoms, int n_geom, const double* x_a, const double* z_a,
               int n_tx, const double* alpha, const double* z_f, int n_rays, double* out8, double* tof4,
               double* tof, double* land_x, uint8_t* status, unsigned flags, int device)
{
    int st = check_shoot(lens, geoms, n_geom, x_a, z_a, n_tx, alpha, z_f, n_rays);
    if (st) return st;
    if (flags & ~RTUS_SHOOT_KNOWN_FLAGS) return RTUS_ERR_INVALID_ARG;
    const size_t rows = (size_t)n_geom * n_tx, n = (size_t)n_rays, rn = rows * n;
    Session S;
    if ((st = S.open(device))) return st;
    // the polyline of an unchanged (alpha, lens) pair is kept in the arena: no polyline launch, no upload of alpha
    Arena& A = *S.a;
    const size_t pw = rtus_ws_bytes(n_rays);
    const bool keep = A.poly_valid && A.poly_ws && A.poly_alpha.size() == n && memcmp(&A.poly_lens, lens, sizeof(rtus_lens)) == 0 &&
                      memcmp(A.poly_alpha.data(), alpha, 8 * n) == 0;
    if (!keep) {
        A.poly_valid = false;
        if (A.poly_cap < pw) {
            if (A.poly_ws) { (void)hipFree(A.poly_ws); A.poly_ws = nullptr; A.poly_cap = 0; }
            HIP_TRY(hipMalloc(&A.poly_ws, pw));
            A.poly_cap = pw;
        }
    }
    double *g, *xa, *za, *al = nullptr, *zf, *o8, *t4, *tt, *lx;
    uint8_t* sb;
    S.in(g, geoms, 2 * (size_t)n_geom);
    S.in(xa, x_a, n_tx);
    S.in(za, z_a, n_tx);
    if (!keep) S.in(al, alpha, n);
    S.in(zf, z_f, n);
    S.out(o8, out8, 8 * rn);
    S.out(t4, tof4, 4 * rn);
    S.out(tt, tof, rn);
    S.out(lx, land_x, rn);
    S.out(sb, status, rn);
    S.allow_direct = true;
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_shoot(*lens, g, n_geom, xa, za, n_tx, al, zf, n_rays, o8, t4, tt, lx, sb, A.poly_ws,
                                 (flags & ~RTUS_POLYLINE_READY) | (keep ? RTUS_POLYLINE_READY : 0u), S.a->stream));
    if ((st = S.finish())) return st;
    if (!keep && n <= ((size_t)1 << 22)) {                  // the call came back clean: the polyline in the arena belongs to this (alpha, lens)
        A.poly_alpha.assign(alpha, alpha + n);
        A.poly_lens = *lens;
        A.poly_valid = true;
    }
    return RTUS_OK;
}

// ---------------------------------------------------------------------------- root-finding solve
size_t rtus_solve_workspace_bytes(int n_rays, int n_geom, int n_tx, int n_rx)
{
    return (n_rays > 0 && n_geom > 0 && n_tx > 0 && n_rx > 0) ? rtus_solve_ws_bytes(n_rays, n_geom, n_tx, n_rx) : 0;
}

static int check_solve(const rtus_lens* lens, const void* geoms, int n_geom, const void* x_a, const void* z_a, int n_tx,
                       const void* alpha, int n_rays, const void* x_rx, int n_rx, double z_land, const void* tt,
                       unsigned flags)
{
    int st = check_shoot(lens, geoms, n_geom, x_a, z_a, n_tx, alpha, alpha, n_rays);
    if (st) return st;
    if (!x_rx || !tt || n_rx <= 0 || !isfinite(z_land)) return RTUS_ERR_INVALID_ARG;
    if (flags & ~(RTUS_SHOOT_KNOWN_FLAGS | RTUS_SOLVE_ONE_LANE | RTUS_SOLVE_THREE_LAUNCHES)) return RTUS_ERR_INVALID_ARG;
    if ((long long)n_geom * n_tx > 0x7fffffffLL / (n_rx > 0 ? n_rx : 1)) return RTUS_ERR_UNSUPPORTED;
    if ((long long)n_geom * n_tx * ((n_rays + 63) / 64) > 0x7fffffffLL) return RTUS_ERR_UNSUPPORTED;
    return RTUS_OK;
}

int rtus_solve_dev(const rtus_lens* lens, const double* d_geoms, int n_geom, const double* d_x_a, const double* d_z_a,
                   int n_tx, const double* d_alpha, int n_rays, const double* d_x_rx, int n_rx, double z_land,
                   double* d_tt, double* d_alpha_root, double* d_tt_all, double* d_alpha_all, uint8_t* d_n_roots,
                   void* d_workspace, size_t workspace_bytes, unsigned flags, void* stream)
{
    int st = check_solve(lens, d_geoms, n_geom, d_x_a, d_z_a, n_tx, d_alpha, n_rays, d_x_rx, n_rx, z_land, d_tt, flags);
    if (st) return st;
    if ((st = check_workspace(d_workspace, workspace_bytes, rtus_solve_ws_bytes(n_rays, n_geom, n_tx, n_rx), 64))) return st;
    LAUNCH_TRY(rtus_launch_solve(*lens, d_geoms, n_geom, d_x_a, d_z_a, n_tx, d_alpha, n_rays, d_x_rx, n_rx, z_land, d_tt,
                              d_alpha_root, d_tt_all, d_alpha_all, d_n_roots, d_workspace, flags, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_solve(const rtus_lens* lens, const double* geoms, int n_geom, const double* x_a, const double* z_a, int n_tx,
               const double* alpha, int n_rays, const double* x_rx, int n_rx, double z_land, double* tt,
               double* alpha_root, double* tt_all, double* alpha_all, uint8_t* n_roots, unsigned flags, int device)
{
    int st = check_solve(lens, geoms, n_geom, x_a, z_a, n_tx, alpha, n_rays, x_rx, n_rx, z_land, tt, flags);
    if (st) return st;
    for (int i = 0; i + 1 < n_rays; ++i)                    // the brackets are intervals of the grid: strictly ascending (host arrays can be checked)
        if (!(alpha[i] < alpha[i + 1])) return RTUS_ERR_INVALID_ARG;
    const size_t tot = (size_t)n_geom * n_tx * n_rx;
    Session S;
    if ((st = S.open(device))) return st;
    double *g, *xa, *za, *al, *rx, *dt, *da, *dta, *daa;
    char* ws;
    uint8_t* dn;
    S.in(g, geoms, 2 * (size_t)n_geom);
    S.in(xa, x_a, n_tx);
    S.in(za, z_a, n_tx);
    S.in(al, alpha, n_rays);
    S.in(rx, x_rx, n_rx);
    S.scratch(ws, rtus_solve_ws_bytes(n_rays, n_geom, n_tx, n_rx));
    S.out(dt, tt, tot);
    S.out(da, alpha_root, tot);
    S.out(dta, tt_all, tot * RTUS_MAX_ROOTS);
    S.out(daa, alpha_all, tot * RTUS_MAX_ROOTS);
    S.out(dn, n_roots, tot);
    S.allow_direct = true;
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_solve(*lens, g, n_geom, xa, za, n_tx, al, n_rays, rx, n_rx, z_land, dt, da, dta, daa, dn, ws,
                              flags & ~RTUS_POLYLINE_READY, S.a->stream));
    return S.finish();
}

// ---------------------------------------------------------------------------- element matcher
static int check_match(const void* land_x, int n_batch, int n_rays, const void* x_rx, int n_rx, double atol,
                       double rtol)
{
    if (!land_x || !x_rx || n_batch <= 0 || n_rays <= 0 || n_rx <= 0) return RTUS_ERR_INVALID_ARG;
    if (!(atol >= 0) || !(rtol >= 0)) return RTUS_ERR_INVALID_ARG;
    if (n_rx > 4000) return RTUS_ERR_UNSUPPORTED;   // x_rx + tolerances live in < 64 KiB of LDS
    return RTUS_OK;
}

int rtus_match_dev(const double* d_land_x, const double* d_tof, int n_batch, int n_rays, const double* d_x_rx,
                   int n_rx, double atol, double rtol, int32_t* d_first_ray, uint8_t* d_hit, double* d_tof_hit,
                   void* stream)
{
    int st = check_match(d_land_x, n_batch, n_rays, d_x_rx, n_rx, atol, rtol);
    if (st) return st;
    if (!d_first_ray) return RTUS_ERR_INVALID_ARG;
    LAUNCH_TRY(rtus_launch_match(d_land_x, d_tof, n_batch, n_rays, d_x_rx, n_rx, atol, rtol, d_first_ray,
                              d_hit, d_tof_hit, nullptr, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_ray_hits_dev(const double* d_land_x, int n_batch, int n_rays, const double* d_x_rx, int n_rx,
                      double atol, double rtol, uint8_t* d_ray_hit, void* stream)
{
    int st = check_match(d_land_x, n_batch, n_rays, d_x_rx, n_rx, atol, rtol);
    if (st) return st;
    if (!d_ray_hit) return RTUS_ERR_INVALID_ARG;
    LAUNCH_TRY(rtus_launch_match(d_land_x, nullptr, n_batch, n_rays, d_x_rx, n_rx, atol, rtol, nullptr,
                              nullptr, nullptr, d_ray_hit, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_match(const double* land_x, const double* tof, int n_batch, int n_rays, const double* x_rx, int n_rx,
               double atol, double rtol, int32_t* first_ray, uint8_t* hit, double* tof_hit, int device)
{
    int st = check_match(land_x, n_batch, n_rays, x_rx, n_rx, atol, rtol);
    if (st) return st;
    if (tof_hit && !tof) return RTUS_ERR_INVALID_ARG;
    const size_t rn = (size_t)n_batch * n_rays, re = (size_t)n_batch * n_rx;
    Session S;
    if ((st = S.open(device))) return st;
    double *lx, *tf = nullptr, *rx, *th;
    int32_t* fr;
    uint8_t* hb;
    S.in(lx, land_x, rn);
    if (tof) S.in(tf, tof, rn);
    S.in(rx, x_rx, n_rx);
    if (first_ray) S.out(fr, first_ray, re);
    else S.scratch(fr, re);                                   // (the matcher writes it whether or not the caller wants it)
    S.out(hb, hit, re);
    S.out(th, tof_hit, re);
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_match(lx, tf, n_batch, n_rays, rx, n_rx, atol, rtol, fr, hb, th, nullptr, S.a->stream));
    return S.finish();
}

int rtus_ray_hits(const double* land_x, int n_batch, int n_rays, const double* x_rx, int n_rx, double atol,
                  double rtol, uint8_t* ray_hit, int device)
{
    int st = check_match(land_x, n_batch, n_rays, x_rx, n_rx, atol, rtol);
    if (st) return st;
    if (!ray_hit) return RTUS_ERR_INVALID_ARG;
    const size_t rn = (size_t)n_batch * n_rays;
    Session S;
    if ((st = S.open(device))) return st;
    double *lx, *rx;
    uint8_t* rh;
    S.in(lx, land_x, rn);
    S.in(rx, x_rx, n_rx);
    S.out(rh, ray_hit, rn);
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_match(lx, nullptr, n_batch, n_rays, rx, n_rx, atol, rtol, nullptr, nullptr, nullptr, rh, S.a->stream));
    return S.finish();
}

// ---------------------------------------------------------------------------- fused sweep (forward trace + matcher)
size_t rtus_sweep_workspace_bytes(int n_rays, int n_geom, int n_tx, int n_rx)
{
    return (n_rays > 0 && n_geom > 0 && n_tx > 0 && n_rx > 0) ? rtus_sweep_ws_bytes(n_rays, n_geom, n_tx, n_rx) : 0;
}

static int check_sweep(const rtus_lens* lens, const void* geoms, int n_geom, const void* x_a, const void* z_a, int n_tx,
                       const void* alpha, const void* z_f, int n_rays, const void* x_rx, int n_rx, double atol, double rtol,
                       const void* first_ray, unsigned flags)
{
    int st = check_shoot(lens, geoms, n_geom, x_a, z_a, n_tx, alpha, z_f, n_rays);
    if (st) return st;
    if (!x_rx || !first_ray || n_rx <= 0 || !(atol >= 0) || !(rtol >= 0)) return RTUS_ERR_INVALID_ARG;
    if (flags & ~RTUS_SHOOT_KNOWN_FLAGS) return RTUS_ERR_INVALID_ARG;
    const long long rows = (long long)n_geom * n_tx, rx_pad = ((long long)n_rx + 63) & ~63LL;
    if (rows * rx_pad + rows > 0x7fffffffLL) return RTUS_ERR_UNSUPPORTED;
    return RTUS_OK;
}

int rtus_sweep_dev(const rtus_lens* lens, const double* d_geoms, int n_geom, const double* d_x_a, const double* d_z_a, int n_tx,
                   const double* d_alpha, const double* d_z_f, int n_rays, const double* d_x_rx, int n_rx, double atol, double rtol,
                   int32_t* d_first_ray, uint8_t* d_hit, double* d_tof_hit, double* d_tof, double* d_land_x, void* d_workspace,
                   size_t workspace_bytes, unsigned flags, void* stream)
{
    int st = check_sweep(lens, d_geoms, n_geom, d_x_a, d_z_a, n_tx, d_alpha, d_z_f, n_rays, d_x_rx, n_rx, atol, rtol, d_first_ray, flags);
    if (st) return st;
    if ((st = check_workspace(d_workspace, workspace_bytes, rtus_sweep_ws_bytes(n_rays, n_geom, n_tx, n_rx), 64))) return st;
    LAUNCH_TRY(rtus_launch_sweep(*lens, d_geoms, n_geom, d_x_a, d_z_a, n_tx, d_alpha, d_z_f, n_rays, d_x_rx, n_rx, atol, rtol, d_first_ray,
                              d_hit, d_tof_hit, d_tof, d_land_x, d_workspace, flags, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_sweep(const rtus_lens* lens, const double* geoms, int n_geom, const double* x_a, const double* z_a, int n_tx,
               const double* alpha, const double* z_f, int n_rays, const double* x_rx, int n_rx, double atol, double rtol,
               int32_t* first_ray, uint8_t* hit, double* tof_hit, double* tof, double* land_x, unsigned flags, int device)
{
    int st = check_sweep(lens, geoms, n_geom, x_a, z_a, n_tx, alpha, z_f, n_rays, x_rx, n_rx, atol, rtol, first_ray, flags);
    if (st) return st;
    const size_t rows = (size_t)n_geom * n_tx, n = (size_t)n_rays, rn = rows * n, re = rows * (size_t)n_rx;
    Session S;
    if ((st = S.open(device))) return st;
    double *g, *xa, *za, *al, *zf, *rx, *th, *tt, *lx;
    char* ws;
    int32_t* fr;
    uint8_t* hb;
    S.in(g, geoms, 2 * (size_t)n_geom);
    S.in(xa, x_a, n_tx);
    S.in(za, z_a, n_tx);
    S.in(al, alpha, n);
    S.in(zf, z_f, n);
    S.in(rx, x_rx, n_rx);
    S.scratch(ws, rtus_sweep_ws_bytes(n_rays, n_geom, n_tx, n_rx));
    S.out(fr, first_ray, re);
    S.out(hb, hit, re);
    S.out(th, tof_hit, re);
    S.out(tt, tof, rn);
    S.out(lx, land_x, rn);
    S.allow_direct = true;
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_sweep(*lens, g, n_geom, xa, za, n_tx, al, zf, n_rays, rx, n_rx, atol, rtol, fr, hb, th, tt, lx, ws,
                              flags & ~RTUS_POLYLINE_READY, S.a->stream));
    return S.finish();
}

// ---------------------------------------------------------------------------- planar layers
static int check_layers(const double* z_if, const double* c, int n_if, const void* xe, const void* ze, int n_e,
                        const void* xf, const void* zf, int n_f, const void* tt)
{
    if (!c || (n_if > 0 && !z_if) || !xe || !ze || !xf || !zf || !tt) return RTUS_ERR_INVALID_ARG;
    if (n_if < 0 || n_e <= 0 || n_f <= 0) return RTUS_ERR_INVALID_ARG;
    if (n_if > RTUS_MAX_LAYERS) return RTUS_ERR_UNSUPPORTED;
    if (n_e > 65535 * 64) return RTUS_ERR_UNSUPPORTED;
    for (int i = 0; i <= n_if; ++i) if (!(c[i] > 0) || !isfinite(c[i])) return RTUS_ERR_INVALID_ARG;
    for (int i = 0; i < n_if; ++i) {
        if (!isfinite(z_if[i])) return RTUS_ERR_INVALID_ARG;
        if (i && !(z_if[i] > z_if[i - 1])) return RTUS_ERR_INVALID_ARG;
    }
    return RTUS_OK;
}

// flags of the planar entries: the accuracy tier; the iteration counts are a diagnostic of the accurate tier's kernel
static int check_tier(unsigned flags, const void* iters)
{
    if (flags & ~RTUS_TT_TAUP_TAIL) return RTUS_ERR_INVALID_ARG;
    if ((flags & RTUS_TT_TAUP_TAIL) && iters) return RTUS_ERR_INVALID_ARG;
    return RTUS_OK;
}

int rtus_tt_layers_ex_dev(const double* z_if, const double* c, int n_if, const double* d_xe, const double* d_ze,
                          int n_e, const double* d_xf, const double* d_zf, int n_f, double* d_tt, uint8_t* d_iters,
                          unsigned flags, void* stream)
{
    int st = check_layers(z_if, c, n_if, d_xe, d_ze, n_e, d_xf, d_zf, n_f, d_tt);
    if (st || (st = check_tier(flags, d_iters))) return st;
    LAUNCH_TRY(rtus_launch_tt_layers(z_if, c, n_if, d_xe, d_ze, n_e, d_xf, d_zf, n_f, d_tt, d_iters, flags,
                                  (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_tt_layers_dev(const double* z_if, const double* c, int n_if, const double* d_xe, const double* d_ze,
                       int n_e, const double* d_xf, const double* d_zf, int n_f, double* d_tt, uint8_t* d_iters,
                       void* stream)
{
    return rtus_tt_layers_ex_dev(z_if, c, n_if, d_xe, d_ze, n_e, d_xf, d_zf, n_f, d_tt, d_iters, 0u, stream);
}

int rtus_tt_layers_batch_ex_dev(const double* z_if, const double* c, int n_if, const double* d_xe, const double* d_ze,
                                int n_e, long long e_stride, const double* d_xf, const double* d_zf, int n_f,
                                long long f_stride, double* d_tt, long long t_stride, int n_batch, unsigned flags, void* stream)
{
    int st = check_layers(z_if, c, n_if, d_xe, d_ze, n_e, d_xf, d_zf, n_f, d_tt);
    if (st || (st = check_tier(flags, nullptr))) return st;
    if (n_batch <= 0 || e_stride < 0 || f_stride < 0) return RTUS_ERR_INVALID_ARG;
    if (n_batch > 1 && t_stride < (long long)n_e * n_f) return RTUS_ERR_INVALID_ARG;   // outputs of two problems would overlap
    if (n_batch > 65535) return RTUS_ERR_UNSUPPORTED;                                   // grid.z
    LAUNCH_TRY(rtus_launch_tt_layers_batch(z_if, c, n_if, d_xe, d_ze, n_e, e_stride, d_xf, d_zf, n_f, f_stride, d_tt,
                                        t_stride, n_batch, flags, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_tt_layers_batch_dev(const double* z_if, const double* c, int n_if, const double* d_xe, const double* d_ze,
                             int n_e, long long e_stride, const double* d_xf, const double* d_zf, int n_f,
                             long long f_stride, double* d_tt, long long t_stride, int n_batch, void* stream)
{
    return rtus_tt_layers_batch_ex_dev(z_if, c, n_if, d_xe, d_ze, n_e, e_stride, d_xf, d_zf, n_f, f_stride, d_tt, t_stride, n_batch, 0u,
                                       stream);
}

size_t rtus_tt_layers_sort_workspace_bytes(int n_e) { return n_e > 0 ? rtus_layers_sort_ws_bytes(n_e) : 0; }

#define RTUS_SORT_MAX_ELEMENTS 32768                 /* the device-side rank is O(n^2) compares */
int rtus_tt_layers_sorted_dev(const double* z_if, const double* c, int n_if, const double* d_xe, const double* d_ze, int n_e,
                              const double* d_xf, const double* d_zf, int n_f, double* d_tt, void* d_workspace, size_t workspace_bytes,
                              unsigned flags, void* stream)
{
    int st = check_layers(z_if, c, n_if, d_xe, d_ze, n_e, d_xf, d_zf, n_f, d_tt);
    if (st) return st;
    if (flags & ~RTUS_TT_TAUP_TAIL) return RTUS_ERR_INVALID_ARG;
    if (n_e > RTUS_SORT_MAX_ELEMENTS) return RTUS_ERR_UNSUPPORTED;
    if ((st = check_workspace(d_workspace, workspace_bytes, rtus_layers_sort_ws_bytes(n_e), 256))) return st;
    LAUNCH_TRY(rtus_launch_tt_layers_sorted(z_if, c, n_if, d_xe, d_ze, n_e, d_xf, d_zf, n_f, d_tt, d_workspace, nullptr, flags,
                                         (hipStream_t)stream));
    return RTUS_OK;
}

// The aperture in (depth, position) order — the order the predictor of the kernel wants; the coordinates are host memory in the
// host-buffer twins, so the sort is the host's: an aperture that arrives in that order (the usual case) goes through unchanged
// (`order` stays empty).  Compared on the IEEE bits made monotone — the key the device-side rank kernel uses — so the order is a
// strict weak order whatever the values (a NaN coordinate sorts last and fails its row only).
static unsigned long long host_order_key(double v)
{
    unsigned long long b;
    memcpy(&b, &v, 8);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
static void aperture_order(const double* xe, const double* ze, int n_e, std::vector<int>& order, std::vector<double>& sx, std::vector<double>& sz)
{
    auto before = [&](int a, int b) {
        const unsigned long long za = host_order_key(ze[a]), zb = host_order_key(ze[b]);
        return za < zb || (za == zb && host_order_key(xe[a]) < host_order_key(xe[b]));
    };
    bool sorted = true;
    for (int i = 1; i < n_e && sorted; ++i) sorted = !before(i, i - 1);
    if (sorted) return;
    order.resize(n_e);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), before);
    sx.resize(n_e); sz.resize(n_e);
    for (int i = 0; i < n_e; ++i) { sx[i] = xe[order[i]]; sz[i] = ze[order[i]]; }
}

int rtus_tt_layers_ex(const double* z_if, const double* c, int n_if, const double* xe, const double* ze, int n_e,
                      const double* xf, const double* zf, int n_f, double* tt, uint8_t* iters, unsigned flags, int device)
{
    int st = check_layers(z_if, c, n_if, xe, ze, n_e, xf, zf, n_f, tt);
    if (st || (st = check_tier(flags, iters))) return st;
    const size_t tot = (size_t)n_e * n_f;
    std::vector<int> order;
    std::vector<double> sx, sz;
    if (!iters) aperture_order(xe, ze, n_e, order, sx, sz);     // (the iteration counts are a diagnostic of the elements AS GIVEN)
    const bool perm = !order.empty();
    Session S;
    if ((st = S.open(device))) return st;
    double *dxe, *dze, *dxf, *dzf, *dtt;
    int* drow = nullptr;
    uint8_t* dit;
    S.in(dxe, perm ? sx.data() : xe, n_e);
    S.in(dze, perm ? sz.data() : ze, n_e);
    S.in(dxf, xf, n_f);
    S.in(dzf, zf, n_f);
    if (perm) S.in(drow, (const int*)order.data(), n_e);
    S.out(dtt, tt, tot);
    S.out(dit, iters, tot);
    if ((st = S.flush())) return st;
    if (perm) LAUNCH_TRY(rtus_launch_tt_layers_sorted(z_if, c, n_if, dxe, dze, n_e, dxf, dzf, n_f, dtt, nullptr, drow, flags, S.a->stream));
    else LAUNCH_TRY(rtus_launch_tt_layers(z_if, c, n_if, dxe, dze, n_e, dxf, dzf, n_f, dtt, dit, flags, S.a->stream));
    return S.finish();
}

int rtus_tt_layers(const double* z_if, const double* c, int n_if, const double* xe, const double* ze, int n_e,
                   const double* xf, const double* zf, int n_f, double* tt, uint8_t* iters, int device)
{
    return rtus_tt_layers_ex(z_if, c, n_if, xe, ze, n_e, xf, zf, n_f, tt, iters, 0u, device);
}

// matrix arrays (three dimensions): rtus_tt_layers's checks + the y vectors, the kernel's own limits, flags = 0
static int check_layers3(const double* z_if, const double* c, int n_if, const void* xe, const void* ye, const void* ze, int n_e,
                         const void* xf, const void* yf, const void* zf, int n_f, const void* tt, unsigned flags)
{
    if (!ye || !yf) return RTUS_ERR_INVALID_ARG;
    const int st = check_layers(z_if, c, n_if, xe, ze, n_e, xf, zf, n_f, tt);
    if (st) return st;
    if (flags) return RTUS_ERR_INVALID_ARG;
    if (n_f >= (1 << 29)) return RTUS_ERR_UNSUPPORTED;                        // a row's byte offsets are 32-bit
    const long long gx = (n_f + RTUS_TT_LAYERS3_POINTS - 1) / RTUS_TT_LAYERS3_POINTS, gy = (n_e + RTUS_TT_LAYERS3_ROWS - 1) / RTUS_TT_LAYERS3_ROWS;
    return gx * gy > 0x7fffffffLL ? RTUS_ERR_UNSUPPORTED : RTUS_OK;           // one workgroup per work item in grid.x
}

int rtus_tt_layers3_dev(const double* z_if, const double* c, int n_if, const double* d_xe, const double* d_ye, const double* d_ze, int n_e,
                        const double* d_xf, const double* d_yf, const double* d_zf, int n_f, double* d_tt, unsigned flags, void* stream)
{
    const int st = check_layers3(z_if, c, n_if, d_xe, d_ye, d_ze, n_e, d_xf, d_yf, d_zf, n_f, d_tt, flags);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_tt_layers3(z_if, c, n_if, d_xe, d_ye, d_ze, n_e, d_xf, d_yf, d_zf, n_f, d_tt, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_tt_layers3(const double* z_if, const double* c, int n_if, const double* xe, const double* ye, const double* ze, int n_e,
                    const double* xf, const double* yf, const double* zf, int n_f, double* tt, unsigned flags, int device)
{
    int st = check_layers3(z_if, c, n_if, xe, ye, ze, n_e, xf, yf, zf, n_f, tt, flags);
    if (st) return st;
    Session S;
    if ((st = S.open(device))) return st;
    double *dxe, *dye, *dze, *dxf, *dyf, *dzf, *dtt;
    S.in(dxe, xe, n_e);
    S.in(dye, ye, n_e);
    S.in(dze, ze, n_e);
    S.in(dxf, xf, n_f);
    S.in(dyf, yf, n_f);
    S.in(dzf, zf, n_f);
    S.out(dtt, tt, (size_t)n_e * n_f);
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_tt_layers3(z_if, c, n_if, dxe, dye, dze, n_e, dxf, dyf, dzf, n_f, dtt, S.a->stream));
    return S.finish();
}

// ---------------------------------------------------------------------------- one curved interface: a sampled profile
#define RTUS_SURFACE_MAX_SAMPLES (1 << 22)
static int check_surface(double x0, double dx, const void* zs, int n_s, double c1, double c2, const void* xe, const void* ze, int n_e,
                         const void* xf, const void* zf, int n_f, const void* tt)
{
    if (!zs || !xe || !ze || !xf || !zf || !tt || n_s < 4 || n_e <= 0 || n_f <= 0) return RTUS_ERR_INVALID_ARG;
    if (!isfinite(x0) || !isfinite(dx) || !(dx > 0) || !isfinite(c1) || !(c1 > 0) || !isfinite(c2) || !(c2 > 0)) return RTUS_ERR_INVALID_ARG;
    if (n_s > RTUS_SURFACE_MAX_SAMPLES || n_e > 65535 * 8) return RTUS_ERR_UNSUPPORTED;   // grid.y: 8 elements per workgroup
    return RTUS_OK;
}

size_t rtus_tt_surface_workspace_bytes(int n_s) { return n_s >= 4 && n_s <= RTUS_SURFACE_MAX_SAMPLES ? rtus_surface_ws_bytes(n_s) : 0; }

int rtus_tt_surface_dev(double x0, double dx, const double* d_zs, int n_s, double c1, double c2, const double* d_xe, const double* d_ze,
                        int n_e, const double* d_xf, const double* d_zf, int n_f, double* d_tt, double* d_x_entry, void* d_workspace,
                        size_t workspace_bytes, void* stream)
{
    int st = check_surface(x0, dx, d_zs, n_s, c1, c2, d_xe, d_ze, n_e, d_xf, d_zf, n_f, d_tt);
    if (st) return st;
    if ((st = check_workspace(d_workspace, workspace_bytes, rtus_surface_ws_bytes(n_s), 256))) return st;
    LAUNCH_TRY(rtus_launch_tt_surface(x0, dx, d_zs, n_s, c1, c2, d_xe, d_ze, n_e, d_xf, d_zf, n_f, d_tt, d_x_entry, d_workspace,
                                      (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_tt_surface(double x0, double dx, const double* zs, int n_s, double c1, double c2, const double* xe, const double* ze, int n_e,
                    const double* xf, const double* zf, int n_f, double* tt, double* x_entry, int device)
{
    int st = check_surface(x0, dx, zs, n_s, c1, c2, xe, ze, n_e, xf, zf, n_f, tt);
    if (st) return st;
    const size_t tot = (size_t)n_e * n_f;
    Session S;
    if ((st = S.open(device))) return st;
    double *dzs, *dxe, *dze, *dxf, *dzf, *dtt, *dxn;
    char* ws;
    S.in(dzs, zs, n_s);
    S.in(dxe, xe, n_e);
    S.in(dze, ze, n_e);
    S.in(dxf, xf, n_f);
    S.in(dzf, zf, n_f);
    S.out(dtt, tt, tot);
    S.out(dxn, x_entry, tot);
    S.scratch(ws, rtus_surface_ws_bytes(n_s));
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_tt_surface(x0, dx, dzs, n_s, c1, c2, dxe, dze, n_e, dxf, dzf, n_f, dtt, dxn, ws, S.a->stream));
    return S.finish();
}

// skip legs through the surface: rtus_tt_surface's checks, c_down in c2's place, and the leg's own speed and backwall
static int check_surface_skip(double x0, double dx, const void* zs, int n_s, double c1, double c_down, double c_up, double z_back,
                              const void* xe, const void* ze, int n_e, const void* xf, const void* zf, int n_f, const void* tt)
{
    if (!isfinite(c_up) || !(c_up > 0) || !isfinite(z_back)) return RTUS_ERR_INVALID_ARG;
    return check_surface(x0, dx, zs, n_s, c1, c_down, xe, ze, n_e, xf, zf, n_f, tt);
}

int rtus_tt_surface_skip_dev(double x0, double dx, const double* d_zs, int n_s, double c1, double c_down, double c_up, double z_back,
                             const double* d_xe, const double* d_ze, int n_e, const double* d_xf, const double* d_zf, int n_f, double* d_tt,
                             double* d_x_entry, double* d_x_back, void* d_workspace, size_t workspace_bytes, void* stream)
{
    int st = check_surface_skip(x0, dx, d_zs, n_s, c1, c_down, c_up, z_back, d_xe, d_ze, n_e, d_xf, d_zf, n_f, d_tt);
    if (st) return st;
    if ((st = check_workspace(d_workspace, workspace_bytes, rtus_surface_ws_bytes(n_s), 256))) return st;
    LAUNCH_TRY(rtus_launch_tt_surface_skip(x0, dx, d_zs, n_s, c1, c_down, c_up, z_back, d_xe, d_ze, n_e, d_xf, d_zf, n_f, d_tt, d_x_entry,
                                           d_x_back, d_workspace, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_tt_surface_skip(double x0, double dx, const double* zs, int n_s, double c1, double c_down, double c_up, double z_back,
                         const double* xe, const double* ze, int n_e, const double* xf, const double* zf, int n_f, double* tt,
                         double* x_entry, double* x_back, int device)
{
    int st = check_surface_skip(x0, dx, zs, n_s, c1, c_down, c_up, z_back, xe, ze, n_e, xf, zf, n_f, tt);
    if (st) return st;
    const size_t tot = (size_t)n_e * n_f;
    Session S;
    if ((st = S.open(device))) return st;
    double *dzs, *dxe, *dze, *dxf, *dzf, *dtt, *dxn, *dxb;
    char* ws;
    S.in(dzs, zs, n_s);
    S.in(dxe, xe, n_e);
    S.in(dze, ze, n_e);
    S.in(dxf, xf, n_f);
    S.in(dzf, zf, n_f);
    S.out(dtt, tt, tot);
    S.out(dxn, x_entry, tot);
    S.out(dxb, x_back, tot);
    S.scratch(ws, rtus_surface_ws_bytes(n_s));
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_tt_surface_skip(x0, dx, dzs, n_s, c1, c_down, c_up, z_back, dxe, dze, n_e, dxf, dzf, n_f, dtt, dxn, dxb, ws,
                                           S.a->stream));
    return S.finish();
}

// ---------------------------------------------------------------------------- an anisotropic part: the group slowness as a series
// rtus_tt_surface's checks (1 / a[0] in c2's place once the series is known to be positive) and the series' own
static int check_aniso_surface(double x0, double dx, const void* zs, int n_s, double c1, const double* a, const double* b, int K,
                               const void* xe, const void* ze, int n_e, const void* xf, const void* zf, int n_f, const void* tt)
{
    if (!rtus_aniso_series_ok(a, b, K)) return RTUS_ERR_INVALID_ARG;
    return check_surface(x0, dx, zs, n_s, c1, 1.0 / a[0], xe, ze, n_e, xf, zf, n_f, tt);
}

int rtus_tt_aniso_surface_dev(double x0, double dx, const double* d_zs, int n_s, double c1, const double* a, const double* b, int K,
                              const double* d_xe, const double* d_ze, int n_e, const double* d_xf, const double* d_zf, int n_f,
                              double* d_tt, double* d_x_entry, void* d_workspace, size_t workspace_bytes, void* stream)
{
    int st = check_aniso_surface(x0, dx, d_zs, n_s, c1, a, b, K, d_xe, d_ze, n_e, d_xf, d_zf, n_f, d_tt);
    if (st) return st;
    if ((st = check_workspace(d_workspace, workspace_bytes, rtus_surface_ws_bytes(n_s), 256))) return st;
    LAUNCH_TRY(rtus_launch_tt_aniso_surface(x0, dx, d_zs, n_s, c1, a, b, K, d_xe, d_ze, n_e, d_xf, d_zf, n_f, d_tt, d_x_entry, d_workspace,
                                            (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_tt_aniso_surface(double x0, double dx, const double* zs, int n_s, double c1, const double* a, const double* b, int K,
                          const double* xe, const double* ze, int n_e, const double* xf, const double* zf, int n_f, double* tt,
                          double* x_entry, int device)
{
    int st = check_aniso_surface(x0, dx, zs, n_s, c1, a, b, K, xe, ze, n_e, xf, zf, n_f, tt);
    if (st) return st;
    const size_t tot = (size_t)n_e * n_f;
    Session S;
    if ((st = S.open(device))) return st;
    double *dzs, *dxe, *dze, *dxf, *dzf, *dtt, *dxn;
    char* ws;
    S.in(dzs, zs, n_s);
    S.in(dxe, xe, n_e);
    S.in(dze, ze, n_e);
    S.in(dxf, xf, n_f);
    S.in(dzf, zf, n_f);
    S.out(dtt, tt, tot);
    S.out(dxn, x_entry, tot);
    S.scratch(ws, rtus_surface_ws_bytes(n_s));
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_tt_aniso_surface(x0, dx, dzs, n_s, c1, a, b, K, dxe, dze, n_e, dxf, dzf, n_f, dtt, dxn, ws, S.a->stream));
    return S.finish();
}

// contact: the probe on the part
static int check_aniso_direct(const double* a, const double* b, int K, const void* xe, const void* ze, int n_e, const void* xf,
                              const void* zf, int n_f, const void* tt)
{
    if (!xe || !ze || !xf || !zf || !tt || n_e <= 0 || n_f <= 0 || !rtus_aniso_series_ok(a, b, K)) return RTUS_ERR_INVALID_ARG;
    return n_e > 65535 ? RTUS_ERR_UNSUPPORTED : RTUS_OK;                      // grid.y: one element per workgroup row
}

int rtus_tt_aniso_direct_dev(const double* a, const double* b, int K, const double* d_xe, const double* d_ze, int n_e, const double* d_xf,
                             const double* d_zf, int n_f, double* d_tt, void* stream)
{
    const int st = check_aniso_direct(a, b, K, d_xe, d_ze, n_e, d_xf, d_zf, n_f, d_tt);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_tt_aniso_direct(a, b, K, d_xe, d_ze, n_e, d_xf, d_zf, n_f, d_tt, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_tt_aniso_direct(const double* a, const double* b, int K, const double* xe, const double* ze, int n_e, const double* xf,
                         const double* zf, int n_f, double* tt, int device)
{
    int st = check_aniso_direct(a, b, K, xe, ze, n_e, xf, zf, n_f, tt);
    if (st) return st;
    Session S;
    if ((st = S.open(device))) return st;
    double *dxe, *dze, *dxf, *dzf, *dtt;
    S.in(dxe, xe, n_e);
    S.in(dze, ze, n_e);
    S.in(dxf, xf, n_f);
    S.in(dzf, zf, n_f);
    S.out(dtt, tt, (size_t)n_e * n_f);
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_tt_aniso_direct(a, b, K, dxe, dze, n_e, dxf, dzf, n_f, dtt, S.a->stream));
    return S.finish();
}

// ---------------------------------------------------------------------------- consumers: focal laws, TFM
static int check_tfm(const void* fmc, int n_tx, int n_rx, int n_t, double fs, double t0, const void* tt_tx, const void* tt_rx,
                     int n_f, const void* image)
{
    if (!fmc || !tt_tx || !tt_rx || !image || n_tx <= 0 || n_rx <= 0 || n_t < 2 || n_f <= 0) return RTUS_ERR_INVALID_ARG;
    if (!(fs > 0) || !isfinite(fs) || !isfinite(t0)) return RTUS_ERR_INVALID_ARG;
    if (n_t > (1 << 28)) return RTUS_ERR_UNSUPPORTED;                 // a record is addressed with 32-bit byte offsets
    return RTUS_OK;
}

int rtus_focal_delays_dev(const double* d_tt, int n_e, int n_f, double* d_delays, void* stream)
{
    if (!d_tt || !d_delays || n_e <= 0 || n_f <= 0) return RTUS_ERR_INVALID_ARG;
    LAUNCH_TRY(rtus_launch_focal_delays(d_tt, n_e, n_f, d_delays, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_focal_delays(const double* tt, int n_e, int n_f, double* delays, int device)
{
    if (!tt || !delays || n_e <= 0 || n_f <= 0) return RTUS_ERR_INVALID_ARG;
    const size_t tot = (size_t)n_e * n_f;
    Session S;
    int st = S.open(device);
    if (st) return st;
    double* d;
    S.in(d, tt, tot);
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_focal_delays(d, n_e, n_f, d, S.a->stream));     // in place: each entry is read before it is written
    S.download(delays, d, tot);
    return S.finish();
}

int rtus_tfm_dev(const float* d_fmc, int n_tx, int n_rx, int n_t, double fs, double t0, const double* d_tt_tx,
                 const double* d_tt_rx, int n_f, float* d_image, void* stream)
{
    int st = check_tfm(d_fmc, n_tx, n_rx, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, d_image);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_tfm(d_fmc, n_tx, n_rx, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, d_image, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_tfm(const float* fmc, int n_tx, int n_rx, int n_t, double fs, double t0, const double* tt_tx, const double* tt_rx,
             int n_f, float* image, int device)
{
    int st = check_tfm(fmc, n_tx, n_rx, n_t, fs, t0, tt_tx, tt_rx, n_f, image);
    if (st) return st;
    const size_t nfmc = (size_t)n_tx * n_rx * n_t;
    const bool same = tt_tx == tt_rx && n_tx == n_rx;
    Session S;
    if ((st = S.open(device))) return st;
    float *dfmc, *dimg;
    double *dtx, *drx = nullptr;
    S.in(dfmc, fmc, nfmc);
    S.in(dtx, tt_tx, (size_t)n_tx * n_f);
    if (!same) S.in(drx, tt_rx, (size_t)n_rx * n_f);
    S.out(dimg, image, n_f);
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_tfm(dfmc, n_tx, n_rx, n_t, fs, t0, dtx, same ? dtx : drx, n_f, dimg, S.a->stream));
    return S.finish();
}

// ---------------------------------------------------------------------------- adaptive TFM: analytic FMC, surface from the couplant image
#define RTUS_ANALYTIC_MAX_TAPS 255
#define RTUS_ANALYTIC_MAX_SAMPLES (1 << 26)
static int check_analytic(const void* fmc, int n_tx, int n_rx, int n_t, int n_taps, const void* out, int in_bytes = 4)   // (2: int16 samples)
{
    if (!fmc || !out || n_tx <= 0 || n_rx <= 0 || n_t <= 0) return RTUS_ERR_INVALID_ARG;
    if (n_taps < 3 || n_taps > RTUS_ANALYTIC_MAX_TAPS || !(n_taps & 1)) return RTUS_ERR_INVALID_ARG;
    if (n_t > RTUS_ANALYTIC_MAX_SAMPLES) return RTUS_ERR_UNSUPPORTED;
    const long long n_pairs = (long long)n_tx * n_rx, n_tiles = (n_t + 1023) / 1024;
    if (n_pairs * n_tiles > 0x7fffffffLL) return RTUS_ERR_UNSUPPORTED;          // one workgroup per (pair, 1024 samples)
    const uintptr_t i0 = (uintptr_t)fmc, i1 = i0 + (uintptr_t)(in_bytes * n_pairs * n_t), o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)(8 * n_pairs * n_t);
    if (i0 < o1 && o0 < i1) return RTUS_ERR_INVALID_ARG;                        // the output must not overlap the input
    return RTUS_OK;
}

int rtus_fmc_analytic_dev(const float* d_fmc, int n_tx, int n_rx, int n_t, int n_taps, float* d_out, void* stream)
{
    int st = check_analytic(d_fmc, n_tx, n_rx, n_t, n_taps, d_out);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_fmc_analytic(d_fmc, (long long)n_tx * n_rx, n_t, n_taps, (float2*)d_out, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_fmc_analytic(const float* fmc, int n_tx, int n_rx, int n_t, int n_taps, float* out, int device)
{
    int st = check_analytic(fmc, n_tx, n_rx, n_t, n_taps, out);
    if (st) return st;
    const size_t n = (size_t)n_tx * n_rx * n_t;
    Session S;
    if ((st = S.open(device))) return st;
    float *din, *dout;
    S.in(din, fmc, n);
    S.out(dout, out, 2 * n);
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_fmc_analytic(din, (long long)n_tx * n_rx, n_t, n_taps, (float2*)dout, S.a->stream));
    return S.finish();
}

#define RTUS_SURFACE_FIND_MAX_E 4096
#define RTUS_SURFACE_FIND_MAX_Z 1024
#define RTUS_SURFACE_FIND_MAX_S (1 << 24)
static int check_surface_find(const void* a, int n_e, int n_t, double fs, double t0, const void* xe, const void* ze, double c1, double x0,
                              double dx, int n_s, double z_lo, double dz, int n_z, const void* z_peak, const void* amp)
{
    if (!a || !xe || !ze || !z_peak || !amp || n_e <= 0 || n_t < 2 || n_s <= 0 || n_z < 3) return RTUS_ERR_INVALID_ARG;
    if (!isfinite(fs) || !(fs > 0) || !isfinite(t0) || !isfinite(c1) || !(c1 > 0)) return RTUS_ERR_INVALID_ARG;
    if (!isfinite(x0) || !isfinite(dx) || !(dx > 0) || !isfinite(z_lo) || !isfinite(dz) || !(dz > 0)) return RTUS_ERR_INVALID_ARG;
    if (n_e > RTUS_SURFACE_FIND_MAX_E || n_z > RTUS_SURFACE_FIND_MAX_Z || n_s > RTUS_SURFACE_FIND_MAX_S || n_t > RTUS_ANALYTIC_MAX_SAMPLES)
        return RTUS_ERR_UNSUPPORTED;
    return RTUS_OK;
}

int rtus_surface_find_dev(const float* d_a, int n_e, int n_t, double fs, double t0, const double* d_xe, const double* d_ze, double c1,
                          double x0, double dx, int n_s, double z_lo, double dz, int n_z, double* d_z_peak, float* d_amp, float* d_image,
                          void* stream)
{
    int st = check_surface_find(d_a, n_e, n_t, fs, t0, d_xe, d_ze, c1, x0, dx, n_s, z_lo, dz, n_z, d_z_peak, d_amp);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_surface_find(d_a, n_e, n_t, fs, t0, d_xe, d_ze, c1, x0, dx, n_s, z_lo, dz, n_z, d_z_peak, d_amp, d_image,
                                        (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_surface_find(const float* a, int n_e, int n_t, double fs, double t0, const double* xe, const double* ze, double c1, double x0,
                      double dx, int n_s, double z_lo, double dz, int n_z, double* z_peak, float* amp, float* image, int device)
{
    int st = check_surface_find(a, n_e, n_t, fs, t0, xe, ze, c1, x0, dx, n_s, z_lo, dz, n_z, z_peak, amp);
    if (st) return st;
    const size_t na = (size_t)n_e * n_e * n_t * 2;
    Session S;
    if ((st = S.open(device))) return st;
    float *da, *damp, *dimg;
    double *dxe, *dze, *dzp;
    S.in(da, a, na);
    S.in(dxe, xe, n_e);
    S.in(dze, ze, n_e);
    S.out(dzp, z_peak, n_s);
    S.out(damp, amp, n_s);
    S.out(dimg, image, (size_t)n_s * n_z);
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_surface_find(da, n_e, n_t, fs, t0, dxe, dze, c1, x0, dx, n_s, z_lo, dz, n_z, dzp, damp, dimg, S.a->stream));
    return S.finish();
}

// ---------------------------------------------------------------------------- echo times of every pair of an analytic FMC
#define RTUS_ECHO_PICK_MAX_PAIRS 0x7fffffffLL
static int check_echo_pick(const void* a, int n_tx, int n_rx, int n_t, double fs, double t0, double t_lo, double t_hi, const void* g_lo,
                           const void* g_hi, const void* t_pick, const void* amp)
{
    if (!a || !t_pick || !amp || n_tx <= 0 || n_rx <= 0 || n_t < 3) return RTUS_ERR_INVALID_ARG;
    if (!isfinite(fs) || !(fs > 0) || !isfinite(t0)) return RTUS_ERR_INVALID_ARG;
    if ((!g_lo && isnan(t_lo)) || (!g_hi && isnan(t_hi))) return RTUS_ERR_INVALID_ARG;   // (infinite: open on that side)
    if ((uintptr_t)a & 7) return RTUS_ERR_INVALID_ARG;                                   // complex samples are read whole
    if (n_t > RTUS_ANALYTIC_MAX_SAMPLES || (long long)n_tx * n_rx > RTUS_ECHO_PICK_MAX_PAIRS) return RTUS_ERR_UNSUPPORTED;
    return RTUS_OK;
}

int rtus_echo_pick_dev(const float* d_a, int n_tx, int n_rx, int n_t, double fs, double t0, double t_lo, double t_hi,
                       const double* d_t_lo, const double* d_t_hi, double* d_t_pick, float* d_amp, void* stream)
{
    int st = check_echo_pick(d_a, n_tx, n_rx, n_t, fs, t0, t_lo, t_hi, d_t_lo, d_t_hi, d_t_pick, d_amp);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_echo_pick(d_a, (long long)n_tx * n_rx, n_t, fs, t0, t_lo, t_hi, d_t_lo, d_t_hi, d_t_pick, d_amp,
                                     (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_echo_pick(const float* a, int n_tx, int n_rx, int n_t, double fs, double t0, double t_lo, double t_hi, const double* g_lo,
                   const double* g_hi, double* t_pick, float* amp, int device)
{
    int st = check_echo_pick(a, n_tx, n_rx, n_t, fs, t0, t_lo, t_hi, g_lo, g_hi, t_pick, amp);
    if (st) return st;
    const size_t n_pairs = (size_t)n_tx * n_rx;
    Session S;
    if ((st = S.open(device))) return st;
    float *da, *damp;
    double *dlo, *dhi, *dt;
    S.in(da, a, n_pairs * n_t * 2);
    S.in(dlo, g_lo, g_lo ? n_pairs : 0);
    S.in(dhi, g_hi, g_hi ? n_pairs : 0);
    S.out(dt, t_pick, n_pairs);
    S.out(damp, amp, n_pairs);
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_echo_pick(da, (long long)n_pairs, n_t, fs, t0, t_lo, t_hi, dlo, dhi, dt, damp, S.a->stream));
    return S.finish();
}

// ---------------------------------------------------------------------------- misfit of a batch of geometries to measured times
#define RTUS_MISFIT_MAX_GEOMS 0x7fffffff
static int check_geom_misfit(const void* tt, int n_geom, int n_tx, int n_rx, const void* t_meas, const void* n, const void* sse,
                             const void* sum_r)
{
    if (!tt || !t_meas || !n || !sse || !sum_r || n_geom <= 0 || n_tx <= 0 || n_rx <= 0) return RTUS_ERR_INVALID_ARG;
    if ((long long)n_tx * n_rx > 0x7fffffffLL) return RTUS_ERR_UNSUPPORTED;             // n[g] is an int
    return RTUS_OK;
}

int rtus_geom_misfit_dev(const double* d_tt, int n_geom, int n_tx, int n_rx, const double* d_t_meas, const double* d_w, int* d_n,
                         double* d_sse, double* d_sum_r, double* d_sum_w, void* stream)
{
    int st = check_geom_misfit(d_tt, n_geom, n_tx, n_rx, d_t_meas, d_n, d_sse, d_sum_r);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_geom_misfit(d_tt, n_geom, n_tx, n_rx, d_t_meas, d_w, d_n, d_sse, d_sum_r, d_sum_w, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_geom_misfit(const double* tt, int n_geom, int n_tx, int n_rx, const double* t_meas, const double* w, int* n, double* sse,
                     double* sum_r, double* sum_w, int device)
{
    int st = check_geom_misfit(tt, n_geom, n_tx, n_rx, t_meas, n, sse, sum_r);
    if (st) return st;
    const size_t row = (size_t)n_tx * n_rx;
    Session S;
    if ((st = S.open(device))) return st;
    double *dtt, *dtm, *dw, *dq, *dr, *dsw;
    int* dn;
    S.in(dtt, tt, row * n_geom);
    S.in(dtm, t_meas, row);
    S.in(dw, w, w ? row : 0);
    S.out(dn, n, n_geom);
    S.out(dq, sse, n_geom);
    S.out(dr, sum_r, n_geom);
    S.out(dsw, sum_w, n_geom);
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_geom_misfit(dtt, n_geom, n_tx, n_rx, dtm, dw, dn, dq, dr, dsw, S.a->stream));
    return S.finish();
}

// ---------------------------------------------------------------------------- specular echo times of sampled reflectors
static int check_specular(const void* tt_a, int n_a, int n_b, int n_refl, int n_p, const void* t)
{
    if (!tt_a || !t || n_a <= 0 || n_b <= 0 || n_refl <= 0 || n_p <= 0) return RTUS_ERR_INVALID_ARG;
    if ((long long)n_refl * n_p > 0x7fffffffLL || (long long)n_a * n_b > 0x7fffffffLL) return RTUS_ERR_UNSUPPORTED;
    if (rtus_specular_blocks(n_a, n_b, n_refl) > 0x7fffffffLL) return RTUS_ERR_UNSUPPORTED;      // one workgroup each, in one grid
    return RTUS_OK;
}

int rtus_specular_dev(const double* d_tt_a, int n_a, const double* d_tt_b, int n_b, int n_refl, int n_p, double* d_t, double* d_pos,
                      int* d_n_min, void* stream)
{
    int st = check_specular(d_tt_a, n_a, n_b, n_refl, n_p, d_t);
    if (st) return st;
    if (!d_tt_b && n_b != n_a) return RTUS_ERR_INVALID_ARG;
    LAUNCH_TRY(rtus_launch_specular(d_tt_a, n_a, d_tt_b, n_b, n_refl, n_p, d_t, d_pos, d_n_min, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_specular(const double* tt_a, int n_a, const double* tt_b, int n_b, int n_refl, int n_p, double* t, double* pos, int* n_min,
                  int device)
{
    int st = check_specular(tt_a, n_a, n_b, n_refl, n_p, t);
    if (st) return st;
    if (!tt_b && n_b != n_a) return RTUS_ERR_INVALID_ARG;
    const size_t cols = (size_t)n_refl * n_p, n_out = (size_t)n_refl * n_a * n_b;
    const bool one = !tt_b || (tt_b == tt_a && n_b == n_a);  // the same table both ways: uploaded once
    Session S;
    if ((st = S.open(device))) return st;
    double *da, *db, *dt, *dp;
    int* dn;
    S.in(da, tt_a, cols * n_a);
    S.in(db, tt_b, one ? 0 : cols * n_b);
    S.out(dt, t, n_out);
    S.out(dp, pos, n_out);
    S.out(dn, n_min, n_out);
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_specular(da, n_a, db, n_b, n_refl, n_p, dt, dp, dn, S.a->stream));
    return S.finish();
}

// ---------------------------------------------------------------------------- skip legs off a sampled backwall
static int check_skip_reflector(const void* tt_down, int n_e, const void* xb, const void* zb, int n_p, double c_up, const void* xf,
                                const void* zf, int n_f, const void* tt)
{
    if (!tt_down || !xb || !zb || !xf || !zf || !tt || n_e <= 0 || n_p <= 0 || n_f <= 0) return RTUS_ERR_INVALID_ARG;
    if (!isfinite(c_up) || !(c_up > 0)) return RTUS_ERR_INVALID_ARG;
    if ((long long)n_e * n_f > 0x7fffffffLL) return RTUS_ERR_UNSUPPORTED;
    if (rtus_skip_reflector_blocks(n_e, n_f) > 0x7fffffffLL) return RTUS_ERR_UNSUPPORTED;        // one workgroup each, in one grid
    return RTUS_OK;
}

int rtus_skip_reflector_dev(const double* d_tt_down, int n_e, const double* d_xb, const double* d_zb, int n_p, double c_up,
                            const double* d_xf, const double* d_zf, int n_f, double* d_tt, double* d_pos, int* d_n_min, void* stream)
{
    int st = check_skip_reflector(d_tt_down, n_e, d_xb, d_zb, n_p, c_up, d_xf, d_zf, n_f, d_tt);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_skip_reflector(d_tt_down, n_e, d_xb, d_zb, n_p, c_up, d_xf, d_zf, n_f, d_tt, d_pos, d_n_min,
                                          (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_skip_reflector(const double* tt_down, int n_e, const double* xb, const double* zb, int n_p, double c_up, const double* xf,
                        const double* zf, int n_f, double* tt, double* pos, int* n_min, int device)
{
    int st = check_skip_reflector(tt_down, n_e, xb, zb, n_p, c_up, xf, zf, n_f, tt);
    if (st) return st;
    const size_t n_out = (size_t)n_e * n_f;
    Session S;
    if ((st = S.open(device))) return st;
    double *dd, *dxb, *dzb, *dxf, *dzf, *dt, *dp;
    int* dn;
    S.in(dd, tt_down, (size_t)n_e * n_p);
    S.in(dxb, xb, n_p);
    S.in(dzb, zb, n_p);
    S.in(dxf, xf, n_f);
    S.in(dzf, zf, n_f);
    S.out(dt, tt, n_out);
    S.out(dp, pos, n_out);
    S.out(dn, n_min, n_out);
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_skip_reflector(dd, n_e, dxb, dzb, n_p, c_up, dxf, dzf, n_f, dt, dp, dn, S.a->stream));
    return S.finish();
}

// ---------------------------------------------------------------------------- FMC simulator: arrivals to A-scans
#define RTUS_SIM_MAX_TABLE 2048                 // n_p + oversample: 16-byte LDS entries, half of a workgroup's 64 KB
#define RTUS_SIM_TILE_SAMPLES 1024              // (rtus_fmcsim.hip: RTUS_SIM_TILE)
static int check_sim(const void* t1, const void* t2, int n_tx, int n_rx, int n, const void* c0, const void* c1, const void* c2,
                     const void* pulse, int n_p, int centre, int os, double fs, double t0, int n_t, const void* out, unsigned flags)
{
    if (!t1 || !t2 || !pulse || !out || n_tx <= 0 || n_rx <= 0 || n <= 0 || n_p <= 0 || n_t <= 0) return RTUS_ERR_INVALID_ARG;
    if (!isfinite(fs) || !(fs > 0) || !isfinite(t0) || os < 1 || centre < 0 || centre >= n_p) return RTUS_ERR_INVALID_ARG;
    if (flags & ~(RTUS_SIM_ANALYTIC | RTUS_SIM_ACCUMULATE)) return RTUS_ERR_INVALID_ARG;
    if ((((uintptr_t)c0 | (uintptr_t)c1 | (uintptr_t)c2 | (uintptr_t)pulse) & 7) || ((uintptr_t)out & 3)) return RTUS_ERR_INVALID_ARG;
    if (n_t > RTUS_ANALYTIC_MAX_SAMPLES || (long long)n_p + os > RTUS_SIM_MAX_TABLE) return RTUS_ERR_UNSUPPORTED;
    const long long n_tiles = (n_t + RTUS_SIM_TILE_SAMPLES - 1) / RTUS_SIM_TILE_SAMPLES;
    if ((long long)n_tx * n_rx * n_tiles > 0x7fffffffLL) return RTUS_ERR_UNSUPPORTED;   // one wave per (pair, 1024 samples)
    return RTUS_OK;
}

int rtus_fmc_sim_dev(const double* d_tt_tx, const double* d_tt_rx, int n_tx, int n_rx, int n_s, const float* d_q, const float* d_w_tx,
                     const float* d_w_rx, const float* d_pulse, int n_p, int centre, int oversample, double fs, double t0, int n_t,
                     float* d_out, unsigned flags, void* stream)
{
    int st = check_sim(d_tt_tx, d_tt_rx, n_tx, n_rx, n_s, d_q, d_w_tx, d_w_rx, d_pulse, n_p, centre, oversample, fs, t0, n_t, d_out, flags);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_fmc_sim(d_tt_tx, d_tt_rx, d_q, d_w_tx, d_w_rx, n_tx, n_rx, n_s, 0, d_pulse, n_p, centre, oversample, fs, t0, n_t,
                                   d_out, !!(flags & RTUS_SIM_ANALYTIC), !!(flags & RTUS_SIM_ACCUMULATE), (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_fmc_sim_echo_dev(const double* d_t_pair, const float* d_amp, int n_tx, int n_rx, int n_a, const float* d_pulse, int n_p,
                          int centre, int oversample, double fs, double t0, int n_t, float* d_out, unsigned flags, void* stream)
{
    int st = check_sim(d_t_pair, d_t_pair, n_tx, n_rx, n_a, d_amp, nullptr, nullptr, d_pulse, n_p, centre, oversample, fs, t0, n_t, d_out,
                       flags);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_fmc_sim(d_t_pair, nullptr, nullptr, d_amp, nullptr, n_tx, n_rx, n_a, 1, d_pulse, n_p, centre, oversample, fs, t0,
                                   n_t, d_out, !!(flags & RTUS_SIM_ANALYTIC), !!(flags & RTUS_SIM_ACCUMULATE), (hipStream_t)stream));
    return RTUS_OK;
}

// the two host twins: `echo` selects which arrays t1 / a1 are (SimArgs in rtus_fmcsim.hip)
static int sim_host(const double* t1, const double* t2, const float* q, const float* a1, const float* a2, int n_tx, int n_rx, int n,
                    int echo, const float* pulse, int n_p, int centre, int os, double fs, double t0, int n_t, float* out, unsigned flags,
                    int device)
{
    const size_t pairs = (size_t)n_tx * n_rx, rows1 = echo ? pairs : (size_t)n_tx;
    const size_t n_out = pairs * n_t * ((flags & RTUS_SIM_ANALYTIC) ? 2 : 1);
    const bool same = !echo && t1 == t2 && n_tx == n_rx, acc = flags & RTUS_SIM_ACCUMULATE;
    Session S;
    int st = S.open(device);
    if (st) return st;
    double *dt1, *dt2 = nullptr;
    float *dq, *da1, *da2, *dp, *dout;
    S.in(dt1, t1, rows1 * n);
    if (!echo && !same) S.in(dt2, t2, (size_t)n_rx * n);
    S.in(dq, q, q ? 2 * (size_t)n : 0);
    S.in(da1, a1, a1 ? 2 * rows1 * n : 0);
    S.in(da2, a2, a2 ? 2 * (size_t)n_rx * n : 0);
    S.in(dp, pulse, 2 * (size_t)n_p);
    if (acc) S.in(dout, (const float*)out, n_out);           // in place: uploaded, added onto, read back
    else S.out(dout, out, n_out);
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_fmc_sim(dt1, echo ? nullptr : (same ? dt1 : dt2), dq, da1, da2, n_tx, n_rx, n, echo, dp, n_p, centre, os, fs, t0,
                                   n_t, dout, !!(flags & RTUS_SIM_ANALYTIC), acc, S.a->stream));
    if (acc) S.download(out, dout, n_out);
    return S.finish();
}

int rtus_fmc_sim(const double* tt_tx, const double* tt_rx, int n_tx, int n_rx, int n_s, const float* q, const float* w_tx,
                 const float* w_rx, const float* pulse, int n_p, int centre, int oversample, double fs, double t0, int n_t, float* out,
                 unsigned flags, int device)
{
    int st = check_sim(tt_tx, tt_rx, n_tx, n_rx, n_s, q, w_tx, w_rx, pulse, n_p, centre, oversample, fs, t0, n_t, out, flags);
    if (st) return st;
    return sim_host(tt_tx, tt_rx, q, w_tx, w_rx, n_tx, n_rx, n_s, 0, pulse, n_p, centre, oversample, fs, t0, n_t, out, flags, device);
}

int rtus_fmc_sim_echo(const double* t_pair, const float* amp, int n_tx, int n_rx, int n_a, const float* pulse, int n_p, int centre,
                      int oversample, double fs, double t0, int n_t, float* out, unsigned flags, int device)
{
    int st = check_sim(t_pair, t_pair, n_tx, n_rx, n_a, amp, nullptr, nullptr, pulse, n_p, centre, oversample, fs, t0, n_t, out, flags);
    if (st) return st;
    return sim_host(t_pair, nullptr, nullptr, amp, nullptr, n_tx, n_rx, n_a, 1, pulse, n_p, centre, oversample, fs, t0, n_t, out, flags,
                    device);
}

// ---------------------------------------------------------------------------- envelope TFM + coherence factor over an analytic FMC
static int check_tfm_analytic(const void* a, int n_tx, int n_rx, int n_t, double fs, double t0, const void* tt_tx, const void* tt_rx,
                              int n_f, const void* image)
{
    int st = check_tfm(a, n_tx, n_rx, n_t, fs, t0, tt_tx, tt_rx, n_f, image);   // (cf is nullable)
    if (st) return st;
    if (n_t > RTUS_ANALYTIC_MAX_SAMPLES) return RTUS_ERR_UNSUPPORTED;           // 16-byte samples, 32-bit byte offsets
    return RTUS_OK;
}

int rtus_tfm_analytic_dev(const float* d_a, int n_tx, int n_rx, int n_t, double fs, double t0, const double* d_tt_tx,
                          const double* d_tt_rx, int n_f, float* d_image, float* d_cf, void* stream)
{
    int st = check_tfm_analytic(d_a, n_tx, n_rx, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, d_image);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_tfm_analytic(d_a, n_tx, n_rx, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, d_image, d_cf, (hipStream_t)stream));
    return RTUS_OK;
}

// the host twins of rtus_tfm_analytic and rtus_tfm_iq: f_demod < 0 stands for the former
static int tfm_analytic_host(const float* a, int n_tx, int n_rx, int n_t, double fs, double t0, double f_demod, const double* tt_tx,
                             const double* tt_rx, int n_f, float* image, float* cf, int device)
{
    int st = check_tfm_analytic(a, n_tx, n_rx, n_t, fs, t0, tt_tx, tt_rx, n_f, image);
    if (st) return st;
    const size_t na = (size_t)n_tx * n_rx * n_t * 2;
    const bool same = tt_tx == tt_rx && n_tx == n_rx;
    Session S;
    if ((st = S.open(device))) return st;
    float *da, *dimg, *dcf;
    double *dtx, *drx = nullptr;
    S.in(da, a, na);
    S.in(dtx, tt_tx, (size_t)n_tx * n_f);
    if (!same) S.in(drx, tt_rx, (size_t)n_rx * n_f);
    S.out(dimg, image, 2 * (size_t)n_f);
    S.out(dcf, cf, n_f);
    if ((st = S.flush())) return st;
    if (f_demod < 0.0) LAUNCH_TRY(rtus_launch_tfm_analytic(da, n_tx, n_rx, n_t, fs, t0, dtx, same ? dtx : drx, n_f, dimg, dcf, S.a->stream));
    else LAUNCH_TRY(rtus_launch_tfm_iq(da, n_tx, n_rx, n_t, fs, t0, f_demod, dtx, same ? dtx : drx, n_f, dimg, dcf, S.a->stream));
    return S.finish();
}

int rtus_tfm_analytic(const float* a, int n_tx, int n_rx, int n_t, double fs, double t0, const double* tt_tx, const double* tt_rx,
                      int n_f, float* image, float* cf, int device)
{
    return tfm_analytic_host(a, n_tx, n_rx, n_t, fs, t0, -1.0, tt_tx, tt_rx, n_f, image, cf, device);
}

// ---------------------------------------------------------------------------- TFM and envelope TFM over a half-matrix capture
#define RTUS_HMC_MAX_ELEMENTS 32768                                   // n_e (n_e + 1) / 2 records fit an int
static int check_tfm_hmc(const void* hmc, int n_e, int n_t, double fs, double t0, const void* tt_tx, const void* tt_rx, int n_f,
                         const void* image, bool analytic)
{
    if (n_e < 1 || n_e > RTUS_HMC_MAX_ELEMENTS) return RTUS_ERR_INVALID_ARG;
    return analytic ? check_tfm_analytic(hmc, n_e, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f, image)
                    : check_tfm(hmc, n_e, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f, image);
}

int rtus_tfm_hmc_dev(const float* d_hmc, int n_e, int n_t, double fs, double t0, const double* d_tt_tx, const double* d_tt_rx, int n_f,
                     float* d_image, void* stream)
{
    int st = check_tfm_hmc(d_hmc, n_e, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, d_image, false);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_tfm_hmc(d_hmc, n_e, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, d_image, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_tfm_analytic_hmc_dev(const float* d_a, int n_e, int n_t, double fs, double t0, const double* d_tt_tx, const double* d_tt_rx,
                              int n_f, float* d_image, float* d_cf, void* stream)
{
    int st = check_tfm_hmc(d_a, n_e, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, d_image, true);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_tfm_analytic_hmc(d_a, n_e, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, d_image, d_cf, (hipStream_t)stream));
    return RTUS_OK;
}

// the two host twins: c = floats per sample (1 real, 2 analytic); cf only with c == 2
static int tfm_hmc_host(const float* hmc, int c, int n_e, int n_t, double fs, double t0, const double* tt_tx, const double* tt_rx,
                        int n_f, float* image, float* cf, int device, double f_demod = -1.0)   // >= 0: rtus_tfm_iq_hmc (c == 2)
{
    int st = check_tfm_hmc(hmc, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f, image, c == 2);
    if (st) return st;
    const size_t n_pairs = (size_t)n_e * ((size_t)n_e + 1) / 2;
    const bool same = tt_tx == tt_rx;
    Session S;
    if ((st = S.open(device))) return st;
    float *dh, *dimg, *dcf = nullptr;
    double *dtx, *drx = nullptr;
    S.in(dh, hmc, n_pairs * n_t * c);
    S.in(dtx, tt_tx, (size_t)n_e * n_f);
    if (!same) S.in(drx, tt_rx, (size_t)n_e * n_f);
    S.out(dimg, image, (size_t)c * n_f);
    if (c == 2) S.out(dcf, cf, n_f);
    if ((st = S.flush())) return st;
    if (c == 2 && f_demod >= 0.0)
        LAUNCH_TRY(rtus_launch_tfm_iq_hmc(dh, n_e, n_t, fs, t0, f_demod, dtx, same ? dtx : drx, n_f, dimg, dcf, S.a->stream));
    else if (c == 2) LAUNCH_TRY(rtus_launch_tfm_analytic_hmc(dh, n_e, n_t, fs, t0, dtx, same ? dtx : drx, n_f, dimg, dcf, S.a->stream));
    else LAUNCH_TRY(rtus_launch_tfm_hmc(dh, n_e, n_t, fs, t0, dtx, same ? dtx : drx, n_f, dimg, S.a->stream));
    return S.finish();
}

int rtus_tfm_hmc(const float* hmc, int n_e, int n_t, double fs, double t0, const double* tt_tx, const double* tt_rx, int n_f,
                 float* image, int device)
{
    return tfm_hmc_host(hmc, 1, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f, image, nullptr, device);
}

int rtus_tfm_analytic_hmc(const float* a, int n_e, int n_t, double fs, double t0, const double* tt_tx, const double* tt_rx, int n_f,
                          float* image, float* cf, int device)
{
    return tfm_hmc_host(a, 2, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f, image, cf, device);
}

// ---------------------------------------------------------------------------- carrier-aware (IQ) envelope TFM, full and half matrix
static int check_f_demod(double f_demod, double fs)
{
    return f_demod >= 0.0 && f_demod < 0.5 * fs ? RTUS_OK : RTUS_ERR_INVALID_ARG;   // (NaN and +inf fail the compares)
}

int rtus_tfm_iq_dev(const float* d_a, int n_tx, int n_rx, int n_t, double fs, double t0, double f_demod, const double* d_tt_tx,
                    const double* d_tt_rx, int n_f, float* d_image, float* d_cf, void* stream)
{
    int st = check_tfm_analytic(d_a, n_tx, n_rx, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, d_image);
    if (!st) st = check_f_demod(f_demod, fs);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_tfm_iq(d_a, n_tx, n_rx, n_t, fs, t0, f_demod, d_tt_tx, d_tt_rx, n_f, d_image, d_cf, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_tfm_iq(const float* a, int n_tx, int n_rx, int n_t, double fs, double t0, double f_demod, const double* tt_tx,
                const double* tt_rx, int n_f, float* image, float* cf, int device)
{
    int st = check_tfm_analytic(a, n_tx, n_rx, n_t, fs, t0, tt_tx, tt_rx, n_f, image);
    if (!st) st = check_f_demod(f_demod, fs);
    if (st) return st;
    return tfm_analytic_host(a, n_tx, n_rx, n_t, fs, t0, f_demod, tt_tx, tt_rx, n_f, image, cf, device);
}

int rtus_tfm_iq_hmc_dev(const float* d_a, int n_e, int n_t, double fs, double t0, double f_demod, const double* d_tt_tx,
                        const double* d_tt_rx, int n_f, float* d_image, float* d_cf, void* stream)
{
    int st = check_tfm_hmc(d_a, n_e, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, d_image, true);
    if (!st) st = check_f_demod(f_demod, fs);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_tfm_iq_hmc(d_a, n_e, n_t, fs, t0, f_demod, d_tt_tx, d_tt_rx, n_f, d_image, d_cf, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_tfm_iq_hmc(const float* a, int n_e, int n_t, double fs, double t0, double f_demod, const double* tt_tx, const double* tt_rx,
                    int n_f, float* image, float* cf, int device)
{
    int st = check_tfm_hmc(a, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f, image, true);
    if (!st) st = check_f_demod(f_demod, fs);
    if (st) return st;
    return tfm_hmc_host(a, 2, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f, image, cf, device, f_demod);
}

// ---------------------------------------------------------------------------- TFM over a stack of frames
size_t rtus_fmc_pack_frames_floats(int n_frames, int n_tx, int n_rx, int n_t)
{
    if (n_frames <= 0 || n_tx <= 0 || n_rx <= 0 || n_t <= 0) return 0;
    const unsigned __int128 n = (unsigned __int128)((n_frames + 1LL) / 2 * 2) * (unsigned)n_tx * (unsigned)n_rx * (unsigned)n_t;
    return n <= ((size_t)1 << 60) ? (size_t)n : 0;                    // (4-byte floats: 2^62 bytes)
}

int rtus_fmc_pack_frames_dev(const float* d_fmc, int n_frames, int n_tx, int n_rx, int n_t, float* d_packed, void* stream)
{
    if (!d_fmc || !d_packed || n_frames <= 0 || n_tx <= 0 || n_rx <= 0 || n_t <= 0) return RTUS_ERR_INVALID_ARG;
    const size_t tot = rtus_fmc_pack_frames_floats(n_frames, n_tx, n_rx, n_t);
    if (!tot) return RTUS_ERR_UNSUPPORTED;
    const size_t n = tot / ((n_frames + 1LL) / 2 * 2);                // floats per frame
    if ((uintptr_t)d_packed & 7) return RTUS_ERR_INVALID_ARG;         // 8-byte stores
    const uintptr_t i0 = (uintptr_t)d_fmc, i1 = i0 + 4 * n * (size_t)n_frames, o0 = (uintptr_t)d_packed, o1 = o0 + 4 * tot;
    if (i0 < o1 && o0 < i1) return RTUS_ERR_INVALID_ARG;              // the output must not overlap the input
    LAUNCH_TRY(rtus_launch_fmc_pack_frames(d_fmc, n_frames, n, d_packed, (hipStream_t)stream));
    return RTUS_OK;
}

// n_slow: the images (RF: pairs of them) of the launch, each ceil(n_f / 256) workgroups
static int check_tfm_frames(const void* data, int n_frames, int n_tx, int n_rx, int n_t, double fs, double t0, const void* tt_tx,
                            const void* tt_rx, int n_f, const void* images, bool pairs)
{
    if (n_frames <= 0) return RTUS_ERR_INVALID_ARG;
    int st = check_tfm_analytic(data, n_tx, n_rx, n_t, fs, t0, tt_tx, tt_rx, n_f, images);   // (16-byte positions in both forms)
    if (st) return st;
    if (rtus_tfm_frames_blocks(pairs ? (int)((n_frames + 1LL) / 2) : n_frames, n_f) > 0x7fffffffLL) return RTUS_ERR_UNSUPPORTED;
    return RTUS_OK;
}

int rtus_tfm_frames_dev(const float* d_packed, int n_frames, int n_tx, int n_rx, int n_t, double fs, double t0, const double* d_tt_tx,
                        const double* d_tt_rx, int n_f, float* d_images, void* stream)
{
    int st = check_tfm_frames(d_packed, n_frames, n_tx, n_rx, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, d_images, true);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_tfm_frames(d_packed, n_frames, n_tx, n_rx, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, d_images, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_tfm_frames(const float* fmc, int n_frames, int n_tx, int n_rx, int n_t, double fs, double t0, const double* tt_tx,
                    const double* tt_rx, int n_f, float* images, int device)
{
    int st = check_tfm_frames(fmc, n_frames, n_tx, n_rx, n_t, fs, t0, tt_tx, tt_rx, n_f, images, true);
    if (st) return st;
    const size_t n = (size_t)n_tx * n_rx * n_t;                       // floats per frame
    const bool same = tt_tx == tt_rx && n_tx == n_rx;
    Session S;
    if ((st = S.open(device))) return st;
    float *dstack, *dpacked, *dimg;
    double *dtx, *drx = nullptr;
    S.in(dstack, fmc, n * n_frames);
    S.in(dtx, tt_tx, (size_t)n_tx * n_f);
    if (!same) S.in(drx, tt_rx, (size_t)n_rx * n_f);
    S.out(dimg, images, (size_t)n_frames * n_f);
    S.scratch(dpacked, rtus_fmc_pack_frames_floats(n_frames, n_tx, n_rx, n_t));
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_fmc_pack_frames(dstack, n_frames, n, dpacked, S.a->stream));
    LAUNCH_TRY(rtus_launch_tfm_frames(dpacked, n_frames, n_tx, n_rx, n_t, fs, t0, dtx, same ? dtx : drx, n_f, dimg, S.a->stream));
    return S.finish();
}

int rtus_tfm_analytic_frames_dev(const float* d_a, int n_frames, int n_tx, int n_rx, int n_t, double fs, double t0, double f_demod,
                                 const double* d_tt_tx, const double* d_tt_rx, int n_f, float* d_images, float* d_cf, void* stream)
{
    int st = check_tfm_frames(d_a, n_frames, n_tx, n_rx, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, d_images, false);
    if (!st) st = check_f_demod(f_demod, fs);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_tfm_analytic_frames(d_a, n_frames, n_tx, n_rx, n_t, fs, t0, f_demod, d_tt_tx, d_tt_rx, n_f, d_images, d_cf,
                                               (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_tfm_analytic_frames(const float* a, int n_frames, int n_tx, int n_rx, int n_t, double fs, double t0, double f_demod,
                             const double* tt_tx, const double* tt_rx, int n_f, float* images, float* cf, int device)
{
    int st = check_tfm_frames(a, n_frames, n_tx, n_rx, n_t, fs, t0, tt_tx, tt_rx, n_f, images, false);
    if (!st) st = check_f_demod(f_demod, fs);
    if (st) return st;
    const bool same = tt_tx == tt_rx && n_tx == n_rx;
    Session S;
    if ((st = S.open(device))) return st;
    float *da, *dimg, *dcf;
    double *dtx, *drx = nullptr;
    S.in(da, a, (size_t)n_frames * n_tx * n_rx * n_t * 2);
    S.in(dtx, tt_tx, (size_t)n_tx * n_f);
    if (!same) S.in(drx, tt_rx, (size_t)n_rx * n_f);
    S.out(dimg, images, 2 * (size_t)n_frames * n_f);
    S.out(dcf, cf, (size_t)n_frames * n_f);
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_tfm_analytic_frames(da, n_frames, n_tx, n_rx, n_t, fs, t0, f_demod, dtx, same ? dtx : drx, n_f, dimg, dcf,
                                               S.a->stream));
    return S.finish();
}

// ---------------------------------------------------------------------------- TFM over a stack of int16 frames
size_t rtus_fmc_pack_frames_i16_words(int n_frames, int n_tx, int n_rx, int n_t)
{
    if (n_frames <= 0 || n_tx <= 0 || n_rx <= 0 || n_t <= 0) return 0;
    const unsigned __int128 n = (unsigned __int128)((n_frames + 3LL) / 4 * 4) * (unsigned)n_tx * (unsigned)n_rx * (unsigned)n_t;
    return n <= ((size_t)1 << 61) ? (size_t)n : 0;                    // (2-byte values: 2^62 bytes)
}

int rtus_fmc_pack_frames_i16_dev(const short* d_fmc, int n_frames, int n_tx, int n_rx, int n_t, short* d_packed, void* stream)
{
    if (!d_fmc || !d_packed || n_frames <= 0 || n_tx <= 0 || n_rx <= 0 || n_t <= 0) return RTUS_ERR_INVALID_ARG;
    const size_t tot = rtus_fmc_pack_frames_i16_words(n_frames, n_tx, n_rx, n_t);
    if (!tot) return RTUS_ERR_UNSUPPORTED;
    const size_t n = tot / ((n_frames + 3LL) / 4 * 4);                // samples per frame
    if (((uintptr_t)d_packed & 7) || ((uintptr_t)d_fmc & 1)) return RTUS_ERR_INVALID_ARG;   // 8-byte stores, 2-byte loads
    const uintptr_t i0 = (uintptr_t)d_fmc, i1 = i0 + 2 * n * (size_t)n_frames, o0 = (uintptr_t)d_packed, o1 = o0 + 2 * tot;
    if (i0 < o1 && o0 < i1) return RTUS_ERR_INVALID_ARG;              // the output must not overlap the input
    LAUNCH_TRY(rtus_launch_fmc_pack_frames_i16(d_fmc, n_frames, n, d_packed, (hipStream_t)stream));
    return RTUS_OK;
}

// check_tfm_frames with the images of a launch counted in quads
static int check_tfm_frames_i16(const void* data, int n_frames, int n_tx, int n_rx, int n_t, double fs, double t0, const void* tt_tx,
                                const void* tt_rx, int n_f, const void* images)
{
    if (n_frames <= 0) return RTUS_ERR_INVALID_ARG;
    int st = check_tfm_analytic(data, n_tx, n_rx, n_t, fs, t0, tt_tx, tt_rx, n_f, images);   // (8-byte positions, 16-byte loads)
    if (st) return st;
    if (rtus_tfm_frames_blocks((int)((n_frames + 3LL) / 4), n_f) > 0x7fffffffLL) return RTUS_ERR_UNSUPPORTED;
    return RTUS_OK;
}

int rtus_tfm_frames_i16_dev(const short* d_packed, int n_frames, int n_tx, int n_rx, int n_t, double fs, double t0, const double* d_tt_tx,
                            const double* d_tt_rx, int n_f, float* d_images, void* stream)
{
    int st = check_tfm_frames_i16(d_packed, n_frames, n_tx, n_rx, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, d_images);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_tfm_frames_i16(d_packed, n_frames, n_tx, n_rx, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, d_images,
                                          (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_tfm_frames_i16(const short* fmc, int n_frames, int n_tx, int n_rx, int n_t, double fs, double t0, const double* tt_tx,
                        const double* tt_rx, int n_f, float* images, int device)
{
    int st = check_tfm_frames_i16(fmc, n_frames, n_tx, n_rx, n_t, fs, t0, tt_tx, tt_rx, n_f, images);
    if (st) return st;
    const size_t n = (size_t)n_tx * n_rx * n_t;                       // samples per frame
    const bool same = tt_tx == tt_rx && n_tx == n_rx;
    Session S;
    if ((st = S.open(device))) return st;
    short *dstack, *dpacked;
    float* dimg;
    double *dtx, *drx = nullptr;
    S.in(dstack, fmc, n * n_frames);
    S.in(dtx, tt_tx, (size_t)n_tx * n_f);
    if (!same) S.in(drx, tt_rx, (size_t)n_rx * n_f);
    S.out(dimg, images, (size_t)n_frames * n_f);
    S.scratch(dpacked, rtus_fmc_pack_frames_i16_words(n_frames, n_tx, n_rx, n_t));
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_fmc_pack_frames_i16(dstack, n_frames, n, dpacked, S.a->stream));
    LAUNCH_TRY(rtus_launch_tfm_frames_i16(dpacked, n_frames, n_tx, n_rx, n_t, fs, t0, dtx, same ? dtx : drx, n_f, dimg, S.a->stream));
    return S.finish();
}

// ---------------------------------------------------------------------------- TFM over a stack of half-matrix frames
// per: frames per block of the packed stack (4: int16 quads, 2: float32 pairs); 8-byte sample positions, 16-byte loads either way
static int check_tfm_frames_hmc(const void* data, int n_frames, int n_e, int n_t, double fs, double t0, const void* tt_tx,
                                const void* tt_rx, int n_f, const void* images, int per)
{
    if (n_frames <= 0) return RTUS_ERR_INVALID_ARG;
    int st = check_tfm_hmc(data, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f, images, true);
    if (st) return st;
    if (rtus_tfm_frames_blocks((int)(((long long)n_frames + per - 1) / per), n_f) > 0x7fffffffLL) return RTUS_ERR_UNSUPPORTED;
    return RTUS_OK;
}

int rtus_tfm_frames_hmc_i16_dev(const short* d_packed, int n_frames, int n_e, int n_t, double fs, double t0, const double* d_tt_tx,
                                const double* d_tt_rx, int n_f, float* d_images, void* stream)
{
    int st = check_tfm_frames_hmc(d_packed, n_frames, n_e, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, d_images, 4);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_tfm_frames_hmc_i16(d_packed, n_frames, n_e, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, d_images, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_tfm_frames_hmc_dev(const float* d_packed, int n_frames, int n_e, int n_t, double fs, double t0, const double* d_tt_tx,
                            const double* d_tt_rx, int n_f, float* d_images, void* stream)
{
    int st = check_tfm_frames_hmc(d_packed, n_frames, n_e, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, d_images, 2);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_tfm_frames_hmc(d_packed, n_frames, n_e, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, d_images, (hipStream_t)stream));
    return RTUS_OK;
}

// the two host twins: the frame-major stack [n_frames][n_pairs][n_t] uploaded in its own type and packed in the arena, the pack
// kernels called with one "transmit row" of n_pairs records (they see n samples per frame only)
static int tfm_frames_hmc_host(const void* hmc, bool i16, int n_frames, int n_e, int n_t, double fs, double t0, const double* tt_tx, const double* tt_rx,
                               int n_f, float* images, int device)
{
    int st = check_tfm_frames_hmc(hmc, n_frames, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f, images, i16 ? 4 : 2);
    if (st) return st;
    const int n_pairs = n_e * (n_e + 1) / 2;                          // (n_e <= RTUS_HMC_MAX_ELEMENTS: fits an int)
    const size_t n = (size_t)n_pairs * n_t;                           // samples per frame
    const size_t words = i16 ? rtus_fmc_pack_frames_i16_words(n_frames, 1, n_pairs, n_t) : rtus_fmc_pack_frames_floats(n_frames, 1, n_pairs, n_t);
    if (!words) return RTUS_ERR_UNSUPPORTED;
    const bool same = tt_tx == tt_rx;
    Session S;
    if ((st = S.open(device))) return st;
    short *dstack16 = nullptr, *dpacked16 = nullptr;
    float *dstack = nullptr, *dpacked = nullptr, *dimg;
    double *dtx, *drx = nullptr;
    if (i16) S.in(dstack16, (const short*)hmc, n * n_frames);
    else S.in(dstack, (const float*)hmc, n * n_frames);
    S.in(dtx, tt_tx, (size_t)n_e * n_f);
    if (!same) S.in(drx, tt_rx, (size_t)n_e * n_f);
    S.out(dimg, images, (size_t)n_frames * n_f);
    if (i16) S.scratch(dpacked16, words);
    else S.scratch(dpacked, words);
    if ((st = S.flush())) return st;
    if (i16) {
        LAUNCH_TRY(rtus_launch_fmc_pack_frames_i16(dstack16, n_frames, n, dpacked16, S.a->stream));
        LAUNCH_TRY(rtus_launch_tfm_frames_hmc_i16(dpacked16, n_frames, n_e, n_t, fs, t0, dtx, same ? dtx : drx, n_f, dimg, S.a->stream));
    } else {
        LAUNCH_TRY(rtus_launch_fmc_pack_frames(dstack, n_frames, n, dpacked, S.a->stream));
        LAUNCH_TRY(rtus_launch_tfm_frames_hmc(dpacked, n_frames, n_e, n_t, fs, t0, dtx, same ? dtx : drx, n_f, dimg, S.a->stream));
    }
    return S.finish();
}

int rtus_tfm_frames_hmc_i16(const short* hmc, int n_frames, int n_e, int n_t, double fs, double t0, const double* tt_tx, const double* tt_rx,
                            int n_f, float* images, int device)
{
    return tfm_frames_hmc_host(hmc, true, n_frames, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f, images, device);
}

int rtus_tfm_frames_hmc(const float* hmc, int n_frames, int n_e, int n_t, double fs, double t0, const double* tt_tx, const double* tt_rx,
                        int n_f, float* images, int device)
{
    return tfm_frames_hmc_host(hmc, false, n_frames, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f, images, device);
}

// ---------------------------------------------------------------------------- envelope TFM over a stack of half-matrix frames
int rtus_fmc_analytic_i16_dev(const short* d_fmc, int n_tx, int n_rx, int n_t, int n_taps, float* d_out, void* stream)
{
    int st = check_analytic(d_fmc, n_tx, n_rx, n_t, n_taps, d_out, 2);
    if (st) return st;
    if (((uintptr_t)d_fmc & 1) || ((uintptr_t)d_out & 7)) return RTUS_ERR_INVALID_ARG;   // 2-byte loads, 8-byte stores
    LAUNCH_TRY(rtus_launch_fmc_analytic_i16(d_fmc, 1, (long long)n_tx * n_rx, n_t, n_taps, false, d_out, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_fmc_analytic_i16(const short* fmc, int n_tx, int n_rx, int n_t, int n_taps, float* out, int device)
{
    int st = check_analytic(fmc, n_tx, n_rx, n_t, n_taps, out, 2);
    if (st) return st;
    const size_t n = (size_t)n_tx * n_rx * n_t;
    Session S;
    if ((st = S.open(device))) return st;
    short* din;
    float* dout;
    S.in(din, fmc, n);
    S.out(dout, out, 2 * n);
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_fmc_analytic_i16(din, 1, (long long)n_tx * n_rx, n_t, n_taps, false, dout, S.a->stream));
    return S.finish();
}

int rtus_fmc_hilbert_pairs_i16_dev(const short* d_fmc, int n_frames, int n_scans, int n_t, int n_taps, float* d_packed, void* stream)
{
    if (!d_fmc || !d_packed || n_frames <= 0 || n_scans <= 0 || n_t <= 0) return RTUS_ERR_INVALID_ARG;
    if (n_taps < 3 || n_taps > RTUS_ANALYTIC_MAX_TAPS || !(n_taps & 1)) return RTUS_ERR_INVALID_ARG;
    if (((uintptr_t)d_fmc & 1) || ((uintptr_t)d_packed & 7)) return RTUS_ERR_INVALID_ARG;   // 2-byte loads, 8-byte stores
    if (n_t > RTUS_ANALYTIC_MAX_SAMPLES) return RTUS_ERR_UNSUPPORTED;
    const long long rows = (n_frames + 1LL) / 2 * n_scans, n_tiles = (n_t + 1023) / 1024;   // one workgroup per (pair, A-scan, 1024 samples)
    if (rows > 0x7fffffffLL || rows * n_tiles > 0x7fffffffLL) return RTUS_ERR_UNSUPPORTED;
    const uintptr_t i0 = (uintptr_t)d_fmc, i1 = i0 + (uintptr_t)(2LL * n_frames * n_scans * n_t);
    const uintptr_t o0 = (uintptr_t)d_packed, o1 = o0 + (uintptr_t)(8 * rows * n_t);
    if (i0 < o1 && o0 < i1) return RTUS_ERR_INVALID_ARG;              // the output must not overlap the input
    LAUNCH_TRY(rtus_launch_fmc_analytic_i16(d_fmc, n_frames, n_scans, n_t, n_taps, true, d_packed, (hipStream_t)stream));
    return RTUS_OK;
}

// The workspace of rtus_tfm_envelope_frames_hmc[_i16]_dev, laid out by ONE function for the size helper and the entries: segments
// at multiples of 256 bytes.  split: the split-plane route (int16, f_demod == 0, no cf) — the quads, the pair-packed Hilbert planes
// and the two sets of image planes; else the complex route — ONE frame's analytic block, reused frame after frame, and with RTUS_ENV_MAGNITUDE the complex images.
struct EnvWork {
    bool split;
    size_t quads, hilbert, re, im;                                    // byte offsets (split)
    size_t analytic, cimages;                                         // byte offsets (complex route)
    size_t bytes;                                                     // 0: a size is not positive, or the sum does not fit 2^62
};
static EnvWork env_work(int n_frames, int n_e, int n_t, int n_f, bool i16, double f_demod, bool want_cf, int flags)
{
    EnvWork w = {};
    if (n_frames <= 0 || n_e < 1 || n_e > RTUS_HMC_MAX_ELEMENTS || n_t <= 0 || n_f <= 0) return w;
    w.split = i16 && f_demod == 0.0 && !want_cf;
    typedef unsigned __int128 u128;
    const u128 n = (u128)((size_t)n_e * ((size_t)n_e + 1) / 2) * (unsigned)n_t;       // samples per frame
    const u128 n_img = (u128)(unsigned)n_frames * (unsigned)n_f;
    u128 end = 0;
    auto seg = [&](size_t& off, u128 bytes) {
        off = end >> 62 ? 0 : (size_t)end;
        end += (bytes + 255) & ~(u128)255;
    };
    if (w.split) {
        seg(w.quads, n * ((unsigned)((n_frames + 3LL) / 4) * 8ULL));
        seg(w.hilbert, n * ((unsigned)((n_frames + 1LL) / 2) * 8ULL));
        seg(w.re, n_img * 4);
        seg(w.im, n_img * 4);
    } else {
        seg(w.analytic, n * 8);
        if (flags & RTUS_ENV_MAGNITUDE) seg(w.cimages, n_img * 8);
    }
    w.bytes = end >> 62 ? 0 : (size_t)end;
    return w;
}

size_t rtus_tfm_envelope_frames_hmc_workspace_bytes(int n_frames, int n_e, int n_t, int n_f, int i16, double f_demod, int want_cf, int flags)
{
    if ((flags & ~RTUS_ENV_MAGNITUDE) || !(f_demod >= 0.0) || !isfinite(f_demod)) return 0;
    return env_work(n_frames, n_e, n_t, n_f, i16 != 0, f_demod, want_cf != 0, flags).bytes;
}

static int check_env_frames(const void* stack, bool i16, int n_frames, int n_e, int n_t, int n_taps, double fs, double t0, double f_demod,
                            const void* tt_tx, const void* tt_rx, int n_f, int flags, const void* images, bool want_cf)
{
    if (n_taps < 3 || n_taps > RTUS_ANALYTIC_MAX_TAPS || !(n_taps & 1) || (flags & ~RTUS_ENV_MAGNITUDE)) return RTUS_ERR_INVALID_ARG;
    if (!(fs > 0) || check_f_demod(f_demod, fs)) return RTUS_ERR_INVALID_ARG;
    const bool split = i16 && f_demod == 0.0 && !want_cf;            // the image kernels' blocks: pairs of frames, or frames
    int st = check_tfm_frames_hmc(stack, n_frames, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f, images, split ? 2 : 1);
    if (st) return st;
    if (((uintptr_t)stack & (i16 ? 1 : 3)) || ((uintptr_t)images & ((flags & RTUS_ENV_MAGNITUDE) ? 3 : 7))) return RTUS_ERR_INVALID_ARG;
    const long long n_pairs = (long long)n_e * (n_e + 1) / 2, n_tiles = (n_t + 1023) / 1024;   // the transformer's grid
    if (n_frames * n_pairs > 0x7fffffffLL || n_frames * n_pairs * n_tiles > 0x7fffffffLL) return RTUS_ERR_UNSUPPORTED;
    return RTUS_OK;
}

// the launches of a call, on device pointers (the _dev entries' and the twins' after their upload)
static int env_frames_run(const void* d_stack, bool i16, int n_frames, int n_e, int n_t, int n_taps, double fs, double t0, double f_demod,
                          const double* d_tt_tx, const double* d_tt_rx, int n_f, int flags, float* d_images, float* d_cf, void* d_work,
                          const EnvWork& w, hipStream_t s)
{
    const int n_pairs = n_e * (n_e + 1) / 2;
    const size_t n = (size_t)n_pairs * n_t, n_img = (size_t)n_frames * n_f;
    const bool mag = flags & RTUS_ENV_MAGNITUDE;
    char* work = (char*)d_work;
    if (w.split) {
        short* quads = (short*)(work + w.quads);
        float *hilbert = (float*)(work + w.hilbert), *re = (float*)(work + w.re), *im = (float*)(work + w.im);
        LAUNCH_TRY(rtus_launch_fmc_pack_frames_i16((const short*)d_stack, n_frames, n, quads, s));
        LAUNCH_TRY(rtus_launch_tfm_frames_hmc_i16(quads, n_frames, n_e, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, re, s));
        LAUNCH_TRY(rtus_launch_fmc_analytic_i16((const short*)d_stack, n_frames, n_pairs, n_t, n_taps, true, hilbert, s));
        LAUNCH_TRY(rtus_launch_tfm_frames_hmc(hilbert, n_frames, n_e, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, im, s));
        LAUNCH_TRY(rtus_launch_envelope_combine(re, im, n_img, mag, d_images, s));
        return RTUS_OK;
    }
    float* an = (float*)(work + w.analytic);
    float* cimages = mag ? (float*)(work + w.cimages) : d_images;
    // Frame by frame: the transformer into the one block, then one launch of rtus_tfm_analytic_hmc's (f_demod > 0: rtus_tfm_iq_hmc's)
    // kernel on it — that entry's bits by construction; the stream orders the block's reuse.  The block (8 B per sample) is gathered
    // while it is still in the last-level cache; with the whole stack transformed first it is not (1.07x / 1.24x of the loop at 256^2
    // with one / two tables: profiles/tfm_envelope_frames_hmc_variants.txt).
    for (int k = 0; k < n_frames; ++k) {
        if (i16) LAUNCH_TRY(rtus_launch_fmc_analytic_i16((const short*)d_stack + (size_t)k * n, 1, n_pairs, n_t, n_taps, false, an, s));
        else LAUNCH_TRY(rtus_launch_fmc_analytic((const float*)d_stack + (size_t)k * n, n_pairs, n_t, n_taps, (float2*)an, s));
        float *img = cimages + (size_t)k * n_f * 2, *cf = d_cf ? d_cf + (size_t)k * n_f : nullptr;
        if (f_demod > 0.0) LAUNCH_TRY(rtus_launch_tfm_iq_hmc(an, n_e, n_t, fs, t0, f_demod, d_tt_tx, d_tt_rx, n_f, img, cf, s));
        else LAUNCH_TRY(rtus_launch_tfm_analytic_hmc(an, n_e, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, img, cf, s));
    }
    if (mag) LAUNCH_TRY(rtus_launch_envelope_combine(cimages, nullptr, n_img, true, d_images, s));
    return RTUS_OK;
}

static int env_frames_dev(const void* d_hmc, bool i16, int n_frames, int n_e, int n_t, int n_taps, double fs, double t0, double f_demod,
                          const double* d_tt_tx, const double* d_tt_rx, int n_f, int flags, float* d_images, float* d_cf, void* d_work,
                          size_t work_bytes, void* stream)
{
    int st = check_env_frames(d_hmc, i16, n_frames, n_e, n_t, n_taps, fs, t0, f_demod, d_tt_tx, d_tt_rx, n_f, flags, d_images, d_cf != nullptr);
    if (st) return st;
    const EnvWork w = env_work(n_frames, n_e, n_t, n_f, i16, f_demod, d_cf != nullptr, flags);
    if (!w.bytes) return RTUS_ERR_UNSUPPORTED;
    if ((st = check_workspace(d_work, work_bytes, w.bytes, 64))) return st;
    return env_frames_run(d_hmc, i16, n_frames, n_e, n_t, n_taps, fs, t0, f_demod, d_tt_tx, d_tt_rx, n_f, flags, d_images, d_cf, d_work, w,
                          (hipStream_t)stream);
}

int rtus_tfm_envelope_frames_hmc_i16_dev(const short* d_hmc, int n_frames, int n_e, int n_t, int n_taps, double fs, double t0, double f_demod,
                                         const double* d_tt_tx, const double* d_tt_rx, int n_f, int flags, float* d_images, float* d_cf,
                                         void* d_work, size_t work_bytes, void* stream)
{
    return env_frames_dev(d_hmc, true, n_frames, n_e, n_t, n_taps, fs, t0, f_demod, d_tt_tx, d_tt_rx, n_f, flags, d_images, d_cf, d_work,
                          work_bytes, stream);
}

int rtus_tfm_envelope_frames_hmc_dev(const float* d_hmc, int n_frames, int n_e, int n_t, int n_taps, double fs, double t0, double f_demod,
                                     const double* d_tt_tx, const double* d_tt_rx, int n_f, int flags, float* d_images, float* d_cf,
                                     void* d_work, size_t work_bytes, void* stream)
{
    return env_frames_dev(d_hmc, false, n_frames, n_e, n_t, n_taps, fs, t0, f_demod, d_tt_tx, d_tt_rx, n_f, flags, d_images, d_cf, d_work,
                          work_bytes, stream);
}

// the two host twins: the frame-major stack uploaded in its own type, the workspace a scratch buffer of the arena
static int env_frames_host(const void* hmc, bool i16, int n_frames, int n_e, int n_t, int n_taps, double fs, double t0, double f_demod,
                           const double* tt_tx, const double* tt_rx, int n_f, int flags, float* images, float* cf, int device)
{
    int st = check_env_frames(hmc, i16, n_frames, n_e, n_t, n_taps, fs, t0, f_demod, tt_tx, tt_rx, n_f, flags, images, cf != nullptr);
    if (st) return st;
    const EnvWork w = env_work(n_frames, n_e, n_t, n_f, i16, f_demod, cf != nullptr, flags);
    if (!w.bytes) return RTUS_ERR_UNSUPPORTED;
    const size_t n = (size_t)n_e * ((size_t)n_e + 1) / 2 * (size_t)n_t * (size_t)n_frames, n_img = (size_t)n_frames * n_f;
    const bool same = tt_tx == tt_rx;
    Session S;
    if ((st = S.open(device))) return st;
    short* dstack16 = nullptr;
    float *dstack = nullptr, *dimg, *dcf;
    double *dtx, *drx = nullptr;
    char* dwork;
    if (i16) S.in(dstack16, (const short*)hmc, n);
    else S.in(dstack, (const float*)hmc, n);
    S.in(dtx, tt_tx, (size_t)n_e * n_f);
    if (!same) S.in(drx, tt_rx, (size_t)n_e * n_f);
    S.out(dimg, images, (flags & RTUS_ENV_MAGNITUDE) ? n_img : 2 * n_img);
    S.out(dcf, cf, n_img);
    S.scratch(dwork, w.bytes);
    if ((st = S.flush())) return st;
    st = env_frames_run(i16 ? (const void*)dstack16 : (const void*)dstack, i16, n_frames, n_e, n_t, n_taps, fs, t0, f_demod, dtx,
                        same ? dtx : drx, n_f, flags, dimg, dcf, dwork, w, S.a->stream);
    if (st) return st;
    return S.finish();
}

int rtus_tfm_envelope_frames_hmc_i16(const short* hmc, int n_frames, int n_e, int n_t, int n_taps, double fs, double t0, double f_demod,
                                     const double* tt_tx, const double* tt_rx, int n_f, int flags, float* images, float* cf, int device)
{
    return env_frames_host(hmc, true, n_frames, n_e, n_t, n_taps, fs, t0, f_demod, tt_tx, tt_rx, n_f, flags, images, cf, device);
}

int rtus_tfm_envelope_frames_hmc(const float* hmc, int n_frames, int n_e, int n_t, int n_taps, double fs, double t0, double f_demod,
                                 const double* tt_tx, const double* tt_rx, int n_f, int flags, float* images, float* cf, int device)
{
    return env_frames_host(hmc, false, n_frames, n_e, n_t, n_taps, fs, t0, f_demod, tt_tx, tt_rx, n_f, flags, images, cf, device);
}

// ---------------------------------------------------------------------------- phase-coherence TFM: vcf, scf
static int check_tfm_phase(const void* a, int n_tx, int n_rx, int n_t, double fs, double t0, const void* tt_tx, const void* tt_rx,
                           int n_f, const void* image)
{
    int st = check_tfm_analytic(a, n_tx, n_rx, n_t, fs, t0, tt_tx, tt_rx, n_f, image);   // (vcf, scf, counts are nullable)
    if (st) return st;
    if ((long long)n_tx * n_rx > (1LL << 30)) return RTUS_ERR_UNSUPPORTED;               // the sign sum is an int32
    return RTUS_OK;
}

int rtus_tfm_phase_dev(const float* d_a, int n_tx, int n_rx, int n_t, double fs, double t0, const double* d_tt_tx,
                       const double* d_tt_rx, int n_f, float* d_image, float* d_vcf, float* d_scf, int* d_counts, void* stream)
{
    int st = check_tfm_phase(d_a, n_tx, n_rx, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, d_image);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_tfm_phase(d_a, n_tx, n_rx, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, d_image, d_vcf, d_scf, d_counts,
                                     (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_tfm_phase(const float* a, int n_tx, int n_rx, int n_t, double fs, double t0, const double* tt_tx, const double* tt_rx,
                   int n_f, float* image, float* vcf, float* scf, int* counts, int device)
{
    int st = check_tfm_phase(a, n_tx, n_rx, n_t, fs, t0, tt_tx, tt_rx, n_f, image);
    if (st) return st;
    const size_t na = (size_t)n_tx * n_rx * n_t * 2;
    const bool same = tt_tx == tt_rx && n_tx == n_rx;
    Session S;
    if ((st = S.open(device))) return st;
    float *da, *dimg, *dvcf, *dscf;
    int* dcnt;
    double *dtx, *drx = nullptr;
    S.in(da, a, na);
    S.in(dtx, tt_tx, (size_t)n_tx * n_f);
    if (!same) S.in(drx, tt_rx, (size_t)n_rx * n_f);
    S.out(dimg, image, 2 * (size_t)n_f);
    S.out(dvcf, vcf, n_f);
    S.out(dscf, scf, n_f);
    S.out(dcnt, counts, 2 * (size_t)n_f);
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_tfm_phase(da, n_tx, n_rx, n_t, fs, t0, dtx, same ? dtx : drx, n_f, dimg, dvcf, dscf, dcnt, S.a->stream));
    return S.finish();
}

// ---------------------------------------------------------------------------- weighted envelope TFM + sensitivity
static int check_tfm_weighted(const void* a, int n_tx, int n_rx, int n_t, double fs, double t0, const void* tt_tx, const void* tt_rx,
                              const void* w_tx, const void* w_rx, int n_f, const void* image)
{
    if (!w_tx || !w_rx) return RTUS_ERR_INVALID_ARG;
    return check_tfm_analytic(a, n_tx, n_rx, n_t, fs, t0, tt_tx, tt_rx, n_f, image);   // (sens is nullable)
}

int rtus_tfm_weighted_dev(const float* d_a, int n_tx, int n_rx, int n_t, double fs, double t0, const double* d_tt_tx,
                          const double* d_tt_rx, const float* d_w_tx, const float* d_w_rx, int n_f, float* d_image, float* d_sens,
                          void* stream)
{
    int st = check_tfm_weighted(d_a, n_tx, n_rx, n_t, fs, t0, d_tt_tx, d_tt_rx, d_w_tx, d_w_rx, n_f, d_image);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_tfm_weighted(d_a, n_tx, n_rx, n_t, fs, t0, d_tt_tx, d_tt_rx, d_w_tx, d_w_rx, n_f, d_image, d_sens,
                                        (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_tfm_weighted(const float* a, int n_tx, int n_rx, int n_t, double fs, double t0, const double* tt_tx, const double* tt_rx,
                      const float* w_tx, const float* w_rx, int n_f, float* image, float* sens, int device)
{
    int st = check_tfm_weighted(a, n_tx, n_rx, n_t, fs, t0, tt_tx, tt_rx, w_tx, w_rx, n_f, image);
    if (st) return st;
    const size_t na = (size_t)n_tx * n_rx * n_t * 2, ntx = (size_t)n_tx * n_f, nrx = (size_t)n_rx * n_f;
    Session S;
    if ((st = S.open(device))) return st;
    float *da, *dwt, *dwr, *dimg, *dsens;
    double *dtx, *drx;
    S.in(da, a, na);
    S.in(dtx, tt_tx, ntx);
    S.in(drx, tt_rx, nrx);
    S.in(dwt, w_tx, 2 * ntx);
    S.in(dwr, w_rx, 2 * nrx);
    S.out(dimg, image, 2 * (size_t)n_f);
    S.out(dsens, sens, n_f);
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_tfm_weighted(da, n_tx, n_rx, n_t, fs, t0, dtx, drx, dwt, dwr, n_f, dimg, dsens, S.a->stream));
    return S.finish();
}

// ---------------------------------------------------------------------------- phase-coherence and weighted TFM over a half matrix
static int check_tfm_phase_hmc(const void* a, int n_e, int n_t, double fs, double t0, const void* tt_tx, const void* tt_rx, int n_f,
                               const void* image)
{
    int st = check_tfm_hmc(a, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f, image, true);         // (vcf, scf, counts are nullable)
    if (st) return st;
    if ((long long)n_e * n_e > (1LL << 30)) return RTUS_ERR_UNSUPPORTED;                 // the sign sum is an int32
    return RTUS_OK;
}

int rtus_tfm_phase_hmc_dev(const float* d_a, int n_e, int n_t, double fs, double t0, const double* d_tt_tx, const double* d_tt_rx,
                           int n_f, float* d_image, float* d_vcf, float* d_scf, int* d_counts, void* stream)
{
    int st = check_tfm_phase_hmc(d_a, n_e, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, d_image);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_tfm_phase_hmc(d_a, n_e, n_t, fs, t0, d_tt_tx, d_tt_rx, n_f, d_image, d_vcf, d_scf, d_counts,
                                         (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_tfm_phase_hmc(const float* a, int n_e, int n_t, double fs, double t0, const double* tt_tx, const double* tt_rx, int n_f,
                       float* image, float* vcf, float* scf, int* counts, int device)
{
    int st = check_tfm_phase_hmc(a, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f, image);
    if (st) return st;
    const size_t n_pairs = (size_t)n_e * ((size_t)n_e + 1) / 2;
    const bool same = tt_tx == tt_rx;
    Session S;
    if ((st = S.open(device))) return st;
    float *da, *dimg, *dvcf, *dscf;
    int* dcnt;
    double *dtx, *drx = nullptr;
    S.in(da, a, n_pairs * n_t * 2);
    S.in(dtx, tt_tx, (size_t)n_e * n_f);
    if (!same) S.in(drx, tt_rx, (size_t)n_e * n_f);
    S.out(dimg, image, 2 * (size_t)n_f);
    S.out(dvcf, vcf, n_f);
    S.out(dscf, scf, n_f);
    S.out(dcnt, counts, 2 * (size_t)n_f);
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_tfm_phase_hmc(da, n_e, n_t, fs, t0, dtx, same ? dtx : drx, n_f, dimg, dvcf, dscf, dcnt, S.a->stream));
    return S.finish();
}

static int check_tfm_weighted_hmc(const void* a, int n_e, int n_t, double fs, double t0, const void* tt_tx, const void* tt_rx,
                                  const void* w_tx, const void* w_rx, int n_f, const void* image)
{
    if (!w_tx || !w_rx) return RTUS_ERR_INVALID_ARG;
    return check_tfm_hmc(a, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f, image, true);           // (sens is nullable)
}

int rtus_tfm_weighted_hmc_dev(const float* d_a, int n_e, int n_t, double fs, double t0, const double* d_tt_tx, const double* d_tt_rx,
                              const float* d_w_tx, const float* d_w_rx, int n_f, float* d_image, float* d_sens, void* stream)
{
    int st = check_tfm_weighted_hmc(d_a, n_e, n_t, fs, t0, d_tt_tx, d_tt_rx, d_w_tx, d_w_rx, n_f, d_image);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_tfm_weighted_hmc(d_a, n_e, n_t, fs, t0, d_tt_tx, d_tt_rx, d_w_tx, d_w_rx, n_f, d_image, d_sens,
                                            (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_tfm_weighted_hmc(const float* a, int n_e, int n_t, double fs, double t0, const double* tt_tx, const double* tt_rx,
                          const float* w_tx, const float* w_rx, int n_f, float* image, float* sens, int device)
{
    int st = check_tfm_weighted_hmc(a, n_e, n_t, fs, t0, tt_tx, tt_rx, w_tx, w_rx, n_f, image);
    if (st) return st;
    const size_t n_pairs = (size_t)n_e * ((size_t)n_e + 1) / 2, n = (size_t)n_e * n_f;
    const bool same = tt_tx == tt_rx, same_w = w_tx == w_rx;          // one upload each; the one-delay-table kernel on `same`
    Session S;
    if ((st = S.open(device))) return st;
    float *da, *dwt, *dwr = nullptr, *dimg, *dsens;
    double *dtx, *drx = nullptr;
    S.in(da, a, n_pairs * n_t * 2);
    S.in(dtx, tt_tx, n);
    if (!same) S.in(drx, tt_rx, n);
    S.in(dwt, w_tx, 2 * n);
    if (!same_w) S.in(dwr, w_rx, 2 * n);
    S.out(dimg, image, 2 * (size_t)n_f);
    S.out(dsens, sens, n_f);
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_tfm_weighted_hmc(da, n_e, n_t, fs, t0, dtx, same ? dtx : drx, dwt, same_w ? dwt : dwr, n_f, dimg, dsens,
                                            S.a->stream));
    return S.finish();
}

// ---------------------------------------------------------------------------- ray amplitude tables through a measured surface
static int check_leg_amp(double x0, double dx, const void* zs, int n_s, double c1, double rho1, double c_l, double c_t, double rho2,
                         double z_back, int leg, int dir, double width, double f_c, const void* xe, const void* ze, int n_e,
                         const void* xf, const void* zf, int n_f, const void* x_entry, const void* x_back, const void* amp)
{
    if (!zs || !xe || !ze || !xf || !zf || !x_entry || !amp || n_s < 4 || n_e <= 0 || n_f <= 0) return RTUS_ERR_INVALID_ARG;
    if (leg < RTUS_LEG_L || leg > RTUS_LEG_TT || (dir != RTUS_AMP_DOWN && dir != RTUS_AMP_UP)) return RTUS_ERR_INVALID_ARG;
    if (leg >= RTUS_LEG_LL && !x_back) return RTUS_ERR_INVALID_ARG;
    if (!isfinite(x0) || !isfinite(dx) || !(dx > 0) || !isfinite(z_back)) return RTUS_ERR_INVALID_ARG;
    const double sp[5] = {c1, rho1, c_l, c_t, rho2};
    for (double v : sp)
        if (!isfinite(v) || !(v > 0)) return RTUS_ERR_INVALID_ARG;
    if (!(c_t < c_l) || !isfinite(width) || width < 0 || (width > 0 && (!isfinite(f_c) || !(f_c > 0)))) return RTUS_ERR_INVALID_ARG;
    if (n_s > RTUS_SURFACE_MAX_SAMPLES || n_e > 65535) return RTUS_ERR_UNSUPPORTED;       // grid.y: one element per row of workgroups
    return RTUS_OK;
}

int rtus_leg_amp_surface_dev(double x0, double dx, const double* d_zs, int n_s, double c1, double rho1, double c_l, double c_t,
                             double rho2, double z_back, int leg, int direction, double element_width, double f_c, const double* d_xe,
                             const double* d_ze, int n_e, const double* d_xf, const double* d_zf, int n_f, const double* d_x_entry,
                             const double* d_x_back, float* d_amp, void* d_workspace, size_t workspace_bytes, void* stream)
{
    int st = check_leg_amp(x0, dx, d_zs, n_s, c1, rho1, c_l, c_t, rho2, z_back, leg, direction, element_width, f_c, d_xe, d_ze, n_e, d_xf,
                           d_zf, n_f, d_x_entry, d_x_back, d_amp);
    if (st) return st;
    if ((st = check_workspace(d_workspace, workspace_bytes, rtus_surface_ws_bytes(n_s), 256))) return st;
    LAUNCH_TRY(rtus_launch_leg_amp_surface(x0, dx, d_zs, n_s, c1, rho1, c_l, c_t, rho2, z_back, leg, direction, element_width, f_c, d_xe,
                                           d_ze, n_e, d_xf, d_zf, n_f, d_x_entry, leg >= RTUS_LEG_LL ? d_x_back : nullptr, d_amp,
                                           d_workspace, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_leg_amp_surface(double x0, double dx, const double* zs, int n_s, double c1, double rho1, double c_l, double c_t, double rho2,
                         double z_back, int leg, int direction, double element_width, double f_c, const double* xe, const double* ze,
                         int n_e, const double* xf, const double* zf, int n_f, const double* x_entry, const double* x_back, float* amp,
                         int device)
{
    int st = check_leg_amp(x0, dx, zs, n_s, c1, rho1, c_l, c_t, rho2, z_back, leg, direction, element_width, f_c, xe, ze, n_e, xf, zf,
                           n_f, x_entry, x_back, amp);
    if (st) return st;
    const bool skip = leg >= RTUS_LEG_LL;
    const size_t tot = (size_t)n_e * n_f;
    Session S;
    if ((st = S.open(device))) return st;
    double *dzs, *dxe, *dze, *dxf, *dzf, *dxn, *dxb = nullptr;
    float* damp;
    char* ws;
    S.in(dzs, zs, n_s);
    S.in(dxe, xe, n_e);
    S.in(dze, ze, n_e);
    S.in(dxf, xf, n_f);
    S.in(dzf, zf, n_f);
    S.in(dxn, x_entry, tot);
    if (skip) S.in(dxb, x_back, tot);
    S.out(damp, amp, 2 * tot);
    S.scratch(ws, rtus_surface_ws_bytes(n_s));
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_leg_amp_surface(x0, dx, dzs, n_s, c1, rho1, c_l, c_t, rho2, z_back, leg, direction, element_width, f_c, dxe, dze,
                                           n_e, dxf, dzf, n_f, dxn, dxb, damp, ws, S.a->stream));
    return S.finish();
}

// ---------------------------------------------------------------------------- plane-wave imaging
#define RTUS_PW_MAX_ANGLES 65535
#define RTUS_SYNTH_MAX_LAWS 65535
#define RTUS_SYNTH_MAX_RX 65535
static int check_aperture(const void* ang, int n_a, double x_lo, double x_hi, double z_a, const void* xf, const void* zf, int n_f,
                          const void* tt)
{
    if (!ang || !xf || !zf || !tt || n_a <= 0 || n_f <= 0) return RTUS_ERR_INVALID_ARG;
    if (!isfinite(x_lo) || !isfinite(x_hi) || !isfinite(z_a) || x_lo > x_hi) return RTUS_ERR_INVALID_ARG;
    if (n_a > RTUS_PW_MAX_ANGLES) return RTUS_ERR_UNSUPPORTED;
    return RTUS_OK;
}

static int check_pw_layers(const double* z_if, const double* c, int n_if, const void* ang, int n_a, double x_lo, double x_hi, double z_a,
                           const void* xf, const void* zf, int n_f, const void* tt)
{
    if (!c || (n_if > 0 && !z_if) || n_if < 0) return RTUS_ERR_INVALID_ARG;
    int st = check_aperture(ang, n_a, x_lo, x_hi, z_a, xf, zf, n_f, tt);
    if (st) return st;
    if (n_if > RTUS_MAX_LAYERS) return RTUS_ERR_UNSUPPORTED;
    for (int i = 0; i <= n_if; ++i) if (!(c[i] > 0) || !isfinite(c[i])) return RTUS_ERR_INVALID_ARG;
    for (int i = 0; i < n_if; ++i) {
        if (!isfinite(z_if[i])) return RTUS_ERR_INVALID_ARG;
        if (i && !(z_if[i] > z_if[i - 1])) return RTUS_ERR_INVALID_ARG;
    }
    if (n_if > 0 && !(z_a < z_if[0])) return RTUS_ERR_INVALID_ARG;
    return RTUS_OK;
}

int rtus_pw_layers_dev(const double* z_if, const double* c, int n_if, const double* d_angles, int n_a, double x_lo, double x_hi,
                       double z_a, const double* d_xf, const double* d_zf, int n_f, double* d_tt, void* stream)
{
    int st = check_pw_layers(z_if, c, n_if, d_angles, n_a, x_lo, x_hi, z_a, d_xf, d_zf, n_f, d_tt);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_pw_layers(z_if, c, n_if, d_angles, n_a, x_lo, x_hi, z_a, d_xf, d_zf, n_f, d_tt, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_pw_layers(const double* z_if, const double* c, int n_if, const double* angles, int n_a, double x_lo, double x_hi, double z_a,
                   const double* xf, const double* zf, int n_f, double* tt, int device)
{
    int st = check_pw_layers(z_if, c, n_if, angles, n_a, x_lo, x_hi, z_a, xf, zf, n_f, tt);
    if (st) return st;
    const size_t tot = (size_t)n_a * n_f;
    Session S;
    if ((st = S.open(device))) return st;
    double *dang, *dxf, *dzf, *dtt;
    S.in(dang, angles, n_a);
    S.in(dxf, xf, n_f);
    S.in(dzf, zf, n_f);
    S.out(dtt, tt, tot);
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_pw_layers(z_if, c, n_if, dang, n_a, x_lo, x_hi, z_a, dxf, dzf, n_f, dtt, S.a->stream));
    return S.finish();
}

static int check_pw_surface(double x0, double dx, const void* zs, int n_s, double c1, double c2, const void* ang, int n_a, double x_lo,
                            double x_hi, double z_a, const void* xf, const void* zf, int n_f, const void* tt)
{
    if (!zs || n_s < 4) return RTUS_ERR_INVALID_ARG;
    if (!isfinite(x0) || !isfinite(dx) || !(dx > 0) || !isfinite(c1) || !(c1 > 0) || !isfinite(c2) || !(c2 > 0)) return RTUS_ERR_INVALID_ARG;
    int st = check_aperture(ang, n_a, x_lo, x_hi, z_a, xf, zf, n_f, tt);
    if (st) return st;
    if (n_s > RTUS_SURFACE_MAX_SAMPLES) return RTUS_ERR_UNSUPPORTED;
    return RTUS_OK;
}

int rtus_pw_surface_dev(double x0, double dx, const double* d_zs, int n_s, double c1, double c2, const double* d_angles, int n_a,
                        double x_lo, double x_hi, double z_a, const double* d_xf, const double* d_zf, int n_f, double* d_tt,
                        double* d_x_entry, void* d_workspace, size_t workspace_bytes, void* stream)
{
    int st = check_pw_surface(x0, dx, d_zs, n_s, c1, c2, d_angles, n_a, x_lo, x_hi, z_a, d_xf, d_zf, n_f, d_tt);
    if (st) return st;
    if ((st = check_workspace(d_workspace, workspace_bytes, rtus_surface_ws_bytes(n_s), 256))) return st;
    LAUNCH_TRY(rtus_launch_pw_surface(x0, dx, d_zs, n_s, c1, c2, d_angles, n_a, x_lo, x_hi, z_a, d_xf, d_zf, n_f, d_tt, d_x_entry,
                                      d_workspace, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_pw_surface(double x0, double dx, const double* zs, int n_s, double c1, double c2, const double* angles, int n_a, double x_lo,
                    double x_hi, double z_a, const double* xf, const double* zf, int n_f, double* tt, double* x_entry, int device)
{
    int st = check_pw_surface(x0, dx, zs, n_s, c1, c2, angles, n_a, x_lo, x_hi, z_a, xf, zf, n_f, tt);
    if (st) return st;
    const size_t tot = (size_t)n_a * n_f;
    Session S;
    if ((st = S.open(device))) return st;
    double *dzs, *dang, *dxf, *dzf, *dtt, *dxn;
    char* ws;
    S.in(dzs, zs, n_s);
    S.in(dang, angles, n_a);
    S.in(dxf, xf, n_f);
    S.in(dzf, zf, n_f);
    S.out(dtt, tt, tot);
    S.out(dxn, x_entry, tot);
    S.scratch(ws, rtus_surface_ws_bytes(n_s));
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_pw_surface(x0, dx, dzs, n_s, c1, c2, dang, n_a, x_lo, x_hi, z_a, dxf, dzf, n_f, dtt, dxn, ws, S.a->stream));
    return S.finish();
}

static int check_synth(const void* fmc, int n_tx, int n_rx, int n_t, double fs, const void* d, int n_v, const void* out)
{
    if (!fmc || !d || !out || n_tx <= 0 || n_rx <= 0 || n_t <= 0 || n_v <= 0) return RTUS_ERR_INVALID_ARG;
    if (!isfinite(fs) || !(fs > 0)) return RTUS_ERR_INVALID_ARG;
    if (n_t > (1 << 28) || n_rx > RTUS_SYNTH_MAX_RX || n_v > RTUS_SYNTH_MAX_LAWS) return RTUS_ERR_UNSUPPORTED;
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)(4 * (size_t)n_v * n_rx * n_t);
    const uintptr_t i0 = (uintptr_t)fmc, i1 = i0 + (uintptr_t)(4 * (size_t)n_tx * n_rx * n_t);
    const uintptr_t d0 = (uintptr_t)d, d1 = d0 + (uintptr_t)(8 * (size_t)n_v * n_tx);
    if ((i0 < o1 && o0 < i1) || (d0 < o1 && o0 < d1)) return RTUS_ERR_INVALID_ARG;   // the output must not overlap an input
    return RTUS_OK;
}

int rtus_fmc_synth_tx_dev(const float* d_fmc, int n_tx, int n_rx, int n_t, double fs, const double* d_delays, int n_v, float* d_out,
                          void* stream)
{
    int st = check_synth(d_fmc, n_tx, n_rx, n_t, fs, d_delays, n_v, d_out);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_fmc_synth_tx(d_fmc, n_tx, n_rx, n_t, fs, d_delays, n_v, d_out, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_fmc_synth_tx(const float* fmc, int n_tx, int n_rx, int n_t, double fs, const double* delays, int n_v, float* out, int device)
{
    int st = check_synth(fmc, n_tx, n_rx, n_t, fs, delays, n_v, out);
    if (st) return st;
    const size_t nin = (size_t)n_tx * n_rx * n_t, nout = (size_t)n_v * n_rx * n_t, nd = (size_t)n_v * n_tx;
    Session S;
    if ((st = S.open(device))) return st;
    float *din, *dout;
    double* dd;
    S.in(din, fmc, nin);
    S.in(dd, delays, nd);
    S.out(dout, out, nout);
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_fmc_synth_tx(din, n_tx, n_rx, n_t, fs, dd, n_v, dout, S.a->stream));
    return S.finish();
}

// ---------------------------------------------------------------------------- curved lens
int rtus_tt_lens_dev(const rtus_lens* lens, double alpha_lo, double alpha_hi, const double* d_xe, const double* d_ze,
                     int n_e, const double* d_xf, const double* d_zf, int n_f, double* d_tt, double* d_alpha_out,
                     void* stream)
{
    int st = check_lens(lens, alpha_lo, alpha_hi, d_xe, d_ze, n_e, d_xf, d_zf, n_f, d_tt);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_tt_lens_f64(*lens, alpha_lo, alpha_hi, d_xe, d_ze, n_e, d_xf, d_zf, n_f, d_tt, d_alpha_out, 0, n_e,
                                    (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_tt_lens_f32_dev(const rtus_lens* lens, double alpha_lo, double alpha_hi, const float* d_xe, const float* d_ze,
                         int n_e, const float* d_xf, const float* d_zf, int n_f, float* d_tt, float* d_alpha_out,
                         void* stream)
{
    int st = check_lens(lens, alpha_lo, alpha_hi, d_xe, d_ze, n_e, d_xf, d_zf, n_f, d_tt);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_tt_lens_f32(*lens, alpha_lo, alpha_hi, d_xe, d_ze, n_e, d_xf, d_zf, n_f, d_tt, d_alpha_out, 0, n_e,
                                    (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_tt_lens(const rtus_lens* lens, double alpha_lo, double alpha_hi, const double* xe, const double* ze, int n_e,
                 const double* xf, const double* zf, int n_f, double* tt, double* alpha_out, int device)
{
    return lens_host<double>(lens, alpha_lo, alpha_hi, xe, ze, n_e, xf, zf, n_f, tt, alpha_out, device,
                             rtus_launch_tt_lens_f64);
}

int rtus_tt_lens_f32(const rtus_lens* lens, double alpha_lo, double alpha_hi, const float* xe, const float* ze,
                     int n_e, const float* xf, const float* zf, int n_f, float* tt, float* alpha_out, int device)
{
    return lens_host<float>(lens, alpha_lo, alpha_hi, xe, ze, n_e, xf, zf, n_f, tt, alpha_out, device,
                            rtus_launch_tt_lens_f32);
}

// ---------------------------------------------------------------------------- row shards of a table, several devices
int rtus_table_rows_per_block(long long n_rows_total, int n_f, int elem_bytes)
{
    if (n_rows_total <= 0 || n_f <= 0 || (elem_bytes != 4 && elem_bytes != 8)) return RTUS_ERR_INVALID_ARG;
    const int eb = rtus_rows_per_block(n_rows_total, n_f, 1, elem_bytes);
    return eb < 1 ? RTUS_ERR_UNSUPPORTED : eb;
}

long long rtus_shard_rows(long long n_rows_total, int n_f, int elem_bytes, int n_shards)
{
    if (n_shards <= 0) return RTUS_ERR_INVALID_ARG;
    const int eb = rtus_table_rows_per_block(n_rows_total, n_f, elem_bytes);
    if (eb < 0) return eb;
    const long long per = (n_rows_total + n_shards - 1) / n_shards;
    return (per + eb - 1) / eb * eb;
}

static int check_rows(int n_rows, long long row0, long long n_rows_total)
{
    if (n_rows <= 0 || row0 < 0 || n_rows_total < row0 + n_rows || n_rows_total > 65535LL * 64) return RTUS_ERR_INVALID_ARG;
    return RTUS_OK;
}

int rtus_tt_layers_rows_dev(const double* z_if, const double* c, int n_if, const double* d_xe, const double* d_ze, int n_rows,
                            long long row0, long long n_rows_total, const double* d_xf, const double* d_zf, int n_f, double* d_tt,
                            unsigned flags, void* stream)
{
    int st = check_layers(z_if, c, n_if, d_xe, d_ze, n_rows, d_xf, d_zf, n_f, d_tt);
    if (st || (st = check_rows(n_rows, row0, n_rows_total))) return st;
    if (flags & ~RTUS_TT_TAUP_TAIL) return RTUS_ERR_INVALID_ARG;
    LAUNCH_TRY(rtus_launch_tt_layers_rows(z_if, c, n_if, d_xe, d_ze, n_rows, (int)row0, n_rows_total, d_xf, d_zf, n_f, d_tt, flags,
                                       (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_tt_lens_rows_dev(const rtus_lens* lens, double alpha_lo, double alpha_hi, const double* d_xe, const double* d_ze, int n_rows,
                          long long row0, long long n_rows_total, const double* d_xf, const double* d_zf, int n_f, double* d_tt,
                          double* d_alpha_out, void* stream)
{
    int st = check_lens(lens, alpha_lo, alpha_hi, d_xe, d_ze, n_rows, d_xf, d_zf, n_f, d_tt);
    if (st || (st = check_rows(n_rows, row0, n_rows_total))) return st;
    LAUNCH_TRY(rtus_launch_tt_lens_f64(*lens, alpha_lo, alpha_hi, d_xe, d_ze, n_rows, d_xf, d_zf, n_f, d_tt, d_alpha_out, (int)row0,
                                    n_rows_total, (hipStream_t)stream));
    return RTUS_OK;
}

int rtus_tt_lens_f32_rows_dev(const rtus_lens* lens, double alpha_lo, double alpha_hi, const float* d_xe, const float* d_ze, int n_rows,
                              long long row0, long long n_rows_total, const float* d_xf, const float* d_zf, int n_f, float* d_tt,
                              float* d_alpha_out, void* stream)
{
    int st = check_lens(lens, alpha_lo, alpha_hi, d_xe, d_ze, n_rows, d_xf, d_zf, n_f, d_tt);
    if (st || (st = check_rows(n_rows, row0, n_rows_total))) return st;
    LAUNCH_TRY(rtus_launch_tt_lens_f32(*lens, alpha_lo, alpha_hi, d_xe, d_ze, n_rows, d_xf, d_zf, n_f, d_tt, d_alpha_out, (int)row0,
                                    n_rows_total, (hipStream_t)stream));
    return RTUS_OK;
}

// How the lens table's rows were solved (diagnostic; tests/test_gpu_irregular_apertures.py): the same launch as
// rtus_tt_lens[_f32]_rows_dev without the alpha output, plus five counters ADDED to d_stats (device memory, 5 x uint64, zeroed by
// the caller), each in wave-elements (one wave = 64 targets of one row): [0] rows that took T alone at the extrapolated start,
// [1] rows solved by one evaluation of T and g, [2] rows that needed the safeguarded iteration, [3] of those, rows that also
// looked at the whole interval (a lane pinned at an end or nearly flat in alpha: two minima may compete), [4] evaluations spent in [2].
int rtus_tt_lens_stats_dev(const rtus_lens* lens, double alpha_lo, double alpha_hi, const double* d_xe, const double* d_ze, int n_rows,
                           long long row0, long long n_rows_total, const double* d_xf, const double* d_zf, int n_f, double* d_tt,
                           unsigned long long* d_stats, void* stream)
{
    int st = check_lens(lens, alpha_lo, alpha_hi, d_xe, d_ze, n_rows, d_xf, d_zf, n_f, d_tt);
    if (st || (st = check_rows(n_rows, row0, n_rows_total))) return st;
    if (!d_stats) return RTUS_ERR_INVALID_ARG;
    LAUNCH_TRY(rtus_launch_tt_lens_f64(*lens, alpha_lo, alpha_hi, d_xe, d_ze, n_rows, d_xf, d_zf, n_f, d_tt, nullptr, (int)row0,
                                    n_rows_total, (hipStream_t)stream, d_stats));
    return RTUS_OK;
}

int rtus_tt_lens_f32_stats_dev(const rtus_lens* lens, double alpha_lo, double alpha_hi, const float* d_xe, const float* d_ze, int n_rows,
                               long long row0, long long n_rows_total, const float* d_xf, const float* d_zf, int n_f, float* d_tt,
                               unsigned long long* d_stats, void* stream)
{
    int st = check_lens(lens, alpha_lo, alpha_hi, d_xe, d_ze, n_rows, d_xf, d_zf, n_f, d_tt);
    if (st || (st = check_rows(n_rows, row0, n_rows_total))) return st;
    if (!d_stats) return RTUS_ERR_INVALID_ARG;
    LAUNCH_TRY(rtus_launch_tt_lens_f32(*lens, alpha_lo, alpha_hi, d_xe, d_ze, n_rows, d_xf, d_zf, n_f, d_tt, nullptr, (int)row0,
                                    n_rows_total, (hipStream_t)stream, d_stats));
    return RTUS_OK;
}

}   // extern "C" (the multi-device host entries share a template)

// One host-buffer call spread over several devices: the table's rows in contiguous blocks (multiples of the table's rows per
// workgroup: every row comes out with the bits the one-device call gives it), one arena + stream per listed device, every
// device copying its block straight into the caller's rows.  No exchange between the devices: a host result needs none.
template <typename R, typename Launch>
static int table_multi(const R* xe, const R* ze, int n_e, const R* xf, const R* zf, int n_f, R* tt, const int* devices, int n_dev,
                       Launch launch)
{
    if (!devices || n_dev <= 0 || n_dev > 64) return RTUS_ERR_INVALID_ARG;
    const long long per = rtus_shard_rows(n_e, n_f, (int)sizeof(R), n_dev);
    if (per < 0) return (int)per;
    // The caller's current device comes back whatever the sessions do: this guard is declared before them, so it is the last to
    // run (each session's own guard restores the device that was current when IT opened — the previous entry of the list).
    DeviceGuard outer;
    { int cur = -1; if (hipGetDevice(&cur) == hipSuccess) outer.prev = cur; }
    std::vector<Session> S(n_dev);
    std::vector<int> live(n_dev, 0), slot(n_dev, 0), ord;
    for (int i = 0; i < n_dev; ++i) {
        for (int j = 0; j < i; ++j) slot[i] += devices[j] == devices[i];
        const long long lo = per * i < n_e ? per * i : n_e, hi = lo + per < n_e ? lo + per : n_e;
        if (hi > lo) ord.push_back(i);
    }
    // arenas are locked in (device, slot) order, whatever the order of the list: two threads calling with [0, 1] and [1, 0]
    // take the two mutexes in the same order
    std::sort(ord.begin(), ord.end(), [&](int a, int b) { return devices[a] != devices[b] ? devices[a] < devices[b] : slot[a] < slot[b]; });
    int st = RTUS_OK;
    for (int i : ord) {                                               // uploads + launches: asynchronous on each device's stream
        const long long lo = per * i, hi = lo + per < n_e ? lo + per : n_e;
        const size_t rows = (size_t)(hi - lo), tot = rows * n_f;
        if ((st = S[i].open(devices[i], slot[i]))) break;
        R *dxe, *dze, *dxf, *dzf, *dtt;
        S[i].in(dxe, xe + lo, rows);
        S[i].in(dze, ze + lo, rows);
        S[i].in(dxf, xf, (size_t)n_f);
        S[i].in(dzf, zf, (size_t)n_f);
        S[i].out(dtt, tt + (size_t)lo * n_f, tot);
        if ((st = S[i].flush())) break;
        (void)hipGetLastError();
        const hipError_t e = launch(dxe, dze, (int)rows, (int)lo, dxf, dzf, dtt, S[i].a->stream);
        if (e != hipSuccess) { st = hip_fail(e); break; }
        live[i] = 1;
    }
    // results back: one host thread per device (a device-to-pageable-host copy occupies its caller; the links are independent)
    std::vector<hipError_t> err(n_dev, hipSuccess);
    std::vector<std::thread> th;
    int mine = -1;
    for (int i = 0; i < n_dev; ++i) {
        if (!live[i]) continue;
        if (mine < 0) { mine = i; continue; }
        th.emplace_back([&, i] { (void)hipSetDevice(S[i].dev_index); err[i] = S[i].copy_back(); });
    }
    if (mine >= 0) { (void)hipSetDevice(S[mine].dev_index); err[mine] = S[mine].copy_back(); }
    for (auto& t : th) t.join();
    for (int i = 0; i < n_dev; ++i) if (st == RTUS_OK && err[i] != hipSuccess) st = hip_fail(err[i]);
    return st;
}

// ---- RCCL, bound at run time (dlopen: librtus.so does not depend on it; a process that already holds PyTorch's librccl
// gets that one) — only the *_multi_dev reassembly needs it
namespace {
typedef struct ncclComm* ncclComm_t;
struct Rccl {
    void* h = nullptr;
    int (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    int (*CommDestroy)(ncclComm_t) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, ncclComm_t, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    std::mutex mu;
    std::vector<int> devs;               // device list of the cached communicators
    std::vector<ncclComm_t> comms;
    bool ok = false;                     // every symbol bound (a library that lacks one stays loaded and unused)
    bool load()
    {
        if (h) return ok;
        for (const char* n : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"})
            if ((h = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
        if (!h) return false;
        CommInitAll = (decltype(CommInitAll))dlsym(h, "ncclCommInitAll");
        CommDestroy = (decltype(CommDestroy))dlsym(h, "ncclCommDestroy");
        AllGather = (decltype(AllGather))dlsym(h, "ncclAllGather");
        GroupStart = (decltype(GroupStart))dlsym(h, "ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))dlsym(h, "ncclGroupEnd");
        return ok = CommInitAll && CommDestroy && AllGather && GroupStart && GroupEnd;
    }
};
Rccl g_rccl;
constexpr int kNcclFloat32 = 7, kNcclFloat64 = 8;   // ncclDataType_t (nccl.h)
}   // namespace

// Each listed device solves its row block INTO its own copy of the (padded) table, d_tt[i] + lo n_f; with `gather` the blocks are
// then exchanged in place by one ncclAllGather per device (single-process communicators, ncclCommInitAll: RCCL over xGMI), so
// every device ends up with the whole table; without it the table stays sharded.  Asynchronous on the given streams.
template <typename R, typename Launch>
static int table_multi_dev(const R* const* d_xe, const R* const* d_ze, int n_e, int n_f, R* const* d_tt, const int* devices, int n_dev,
                           void* const* streams, int gather, Launch launch)
{
    if (!d_xe || !d_ze || !d_tt || !devices || !streams || n_dev <= 0 || n_dev > 64) return RTUS_ERR_INVALID_ARG;
    const long long per = rtus_shard_rows(n_e, n_f, (int)sizeof(R), n_dev);
    if (per < 0) return (int)per;
    DeviceGuard guard;
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess) guard.prev = cur;
    for (int i = 0; i < n_dev; ++i) {
        const long long lo = per * i < n_e ? per * i : n_e, hi = lo + per < n_e ? lo + per : n_e;
        if (hi <= lo) continue;
        if (!d_xe[i] || !d_ze[i] || !d_tt[i]) return RTUS_ERR_INVALID_ARG;
        HIP_TRY(hipSetDevice(devices[i]));
        (void)hipGetLastError();
        HIP_TRY(launch(i, d_xe[i] + lo, d_ze[i] + lo, (int)(hi - lo), (int)lo, d_tt[i] + (size_t)lo * n_f, (hipStream_t)streams[i]));
    }
    if (!gather || n_dev == 1) return RTUS_OK;
    std::lock_guard<std::mutex> lk(g_rccl.mu);
    if (!g_rccl.load()) return RTUS_ERR_UNSUPPORTED;
    if (g_rccl.devs != std::vector<int>(devices, devices + n_dev)) {
        // communicators of another device list: collectives of an earlier asynchronous call may still be queued on them
        for (size_t k = 0; k < g_rccl.comms.size(); ++k) {
            if (k < g_rccl.devs.size() && hipSetDevice(g_rccl.devs[k]) == hipSuccess) (void)hipDeviceSynchronize();
            if (g_rccl.comms[k]) (void)g_rccl.CommDestroy(g_rccl.comms[k]);
        }
        g_rccl.comms.assign(n_dev, nullptr);
        g_rccl.devs.clear();
        if (g_rccl.CommInitAll(g_rccl.comms.data(), n_dev, devices) != 0) { g_rccl.comms.clear(); return RTUS_ERR_UNSUPPORTED; }
        g_rccl.devs.assign(devices, devices + n_dev);
    }
    int bad = g_rccl.GroupStart();
    if (bad) return RTUS_ERR_UNSUPPORTED;
    for (int i = 0; i < n_dev && !bad; ++i) {
        if (hipSetDevice(devices[i]) != hipSuccess) { bad = 1; break; }       // (the group is closed below on every path)
        bad = g_rccl.AllGather(d_tt[i] + (size_t)per * i * n_f, d_tt[i], (size_t)per * n_f, sizeof(R) == 8 ? kNcclFloat64 : kNcclFloat32,
                               g_rccl.comms[i], (hipStream_t)streams[i]);
    }
    bad |= g_rccl.GroupEnd();
    return bad ? RTUS_ERR_UNSUPPORTED : RTUS_OK;
}

extern "C" {

int rtus_tt_layers_multi_ex(const double* z_if, const double* c, int n_if, const double* xe, const double* ze, int n_e, const double* xf,
                            const double* zf, int n_f, double* tt, const int* devices, int n_dev, unsigned flags)
{
    int st = check_layers(z_if, c, n_if, xe, ze, n_e, xf, zf, n_f, tt);
    if (st || (st = check_tier(flags, nullptr))) return st;
    // as the one-device twin: the aperture in (depth, position) order first, so that an element's bits do not depend on the order
    // it was handed over in and the table is the one-device table whatever that order.  The shards are blocks of the SORTED rows;
    // they come back into a staging table and every row is copied where it belongs.
    std::vector<int> order;
    std::vector<double> sx, sz, staged;
    aperture_order(xe, ze, n_e, order, sx, sz);
    const bool perm = !order.empty();
    if (perm) staged.resize((size_t)n_e * n_f);
    st = table_multi<double>(perm ? sx.data() : xe, perm ? sz.data() : ze, n_e, xf, zf, n_f, perm ? staged.data() : tt, devices, n_dev,
                             [&](const double* dxe, const double* dze, int rows, int row0, const double* dxf, const double* dzf, double* dtt,
                                 hipStream_t s) { return rtus_launch_tt_layers_rows(z_if, c, n_if, dxe, dze, rows, row0, n_e, dxf, dzf, n_f, dtt, flags, s); });
    if (st == RTUS_OK && perm)
        for (int i = 0; i < n_e; ++i) memcpy(tt + (size_t)order[i] * n_f, staged.data() + (size_t)i * n_f, sizeof(double) * (size_t)n_f);
    return st;
}

int rtus_tt_layers_multi(const double* z_if, const double* c, int n_if, const double* xe, const double* ze, int n_e, const double* xf,
                         const double* zf, int n_f, double* tt, const int* devices, int n_dev)
{
    return rtus_tt_layers_multi_ex(z_if, c, n_if, xe, ze, n_e, xf, zf, n_f, tt, devices, n_dev, 0u);
}

int rtus_tt_lens_f32_multi(const rtus_lens* lens, double alpha_lo, double alpha_hi, const float* xe, const float* ze, int n_e,
                           const float* xf, const float* zf, int n_f, float* tt, const int* devices, int n_dev)
{
    int st = check_lens(lens, alpha_lo, alpha_hi, xe, ze, n_e, xf, zf, n_f, tt);
    if (st) return st;
    return table_multi<float>(xe, ze, n_e, xf, zf, n_f, tt, devices, n_dev,
                              [&](const float* dxe, const float* dze, int rows, int row0, const float* dxf, const float* dzf, float* dtt,
                                  hipStream_t s) {
                                  return rtus_launch_tt_lens_f32(*lens, alpha_lo, alpha_hi, dxe, dze, rows, dxf, dzf, n_f, dtt, nullptr, row0, n_e, s);
                              });
}

int rtus_tt_layers_multi_ex_dev(const double* z_if, const double* c, int n_if, const double* const* d_xe, const double* const* d_ze, int n_e,
                                const double* const* d_xf, const double* const* d_zf, int n_f, double* const* d_tt, const int* devices,
                                int n_dev, void* const* streams, int gather, unsigned flags)
{
    if (!d_xf || !d_zf || !d_xe || !d_ze || !d_tt || n_dev <= 0) return RTUS_ERR_INVALID_ARG;
    int st = check_layers(z_if, c, n_if, d_xe[0], d_ze[0], n_e, d_xf[0], d_zf[0], n_f, d_tt[0]);
    if (st || (st = check_tier(flags, nullptr))) return st;
    return table_multi_dev<double>(d_xe, d_ze, n_e, n_f, d_tt, devices, n_dev, streams, gather,
                                   [&](int i, const double* xe, const double* ze, int rows, int row0, double* tt, hipStream_t s) {
                                       return rtus_launch_tt_layers_rows(z_if, c, n_if, xe, ze, rows, row0, n_e, d_xf[i], d_zf[i], n_f, tt, flags, s);
                                   });
}

int rtus_tt_layers_multi_dev(const double* z_if, const double* c, int n_if, const double* const* d_xe, const double* const* d_ze, int n_e,
                             const double* const* d_xf, const double* const* d_zf, int n_f, double* const* d_tt, const int* devices,
                             int n_dev, void* const* streams, int gather)
{
    return rtus_tt_layers_multi_ex_dev(z_if, c, n_if, d_xe, d_ze, n_e, d_xf, d_zf, n_f, d_tt, devices, n_dev, streams, gather, 0u);
}

int rtus_tt_lens_f32_multi_dev(const rtus_lens* lens, double alpha_lo, double alpha_hi, const float* const* d_xe, const float* const* d_ze,
                               int n_e, const float* const* d_xf, const float* const* d_zf, int n_f, float* const* d_tt,
                               const int* devices, int n_dev, void* const* streams, int gather)
{
    if (!d_xf || !d_zf || !d_xe || !d_ze || !d_tt || n_dev <= 0) return RTUS_ERR_INVALID_ARG;
    int st = check_lens(lens, alpha_lo, alpha_hi, d_xe[0], d_ze[0], n_e, d_xf[0], d_zf[0], n_f, d_tt[0]);
    if (st) return st;
    return table_multi_dev<float>(d_xe, d_ze, n_e, n_f, d_tt, devices, n_dev, streams, gather,
                                  [&](int i, const float* xe, const float* ze, int rows, int row0, float* tt, hipStream_t s) {
                                      return rtus_launch_tt_lens_f32(*lens, alpha_lo, alpha_hi, xe, ze, rows, d_xf[i], d_zf[i], n_f, tt, nullptr,
                                                                     row0, n_e, s);
                                  });
}

}   // extern "C"

// ---------------------------------------------------------------------------- lens -> pipe wall
// The least distance from the pipe's centre to the lens surface over [a_lo, a_hi] (h(alpha): main_rt.py:180-189, root [1]):
// 4097 even samples, then golden-section search on the cells either side of the least one.  Samples where the lens is not
// defined (NaN) do not count.
static double lens_clearance(const rtus_lens& L, double a_lo, double a_hi, double x_off)
{
    const double T = L.l0 / L.c1 + L.h0 / L.c2, c1sq = L.c1 * L.c1;
    const double A = c1sq / (L.c2 * L.c2) - 1.0, C = c1sq * (T * T) - L.d * L.d;
    auto dist = [&](double al) {
        const double B = 2.0 * L.d * cos(al) - 2.0 * T * c1sq / L.c2;
        const double h = (-B - sqrt(B * B - 4.0 * A * C)) / (2.0 * A);
        const double px = h * sin(al) - x_off, pz = h * cos(al);
        return sqrt(px * px + pz * pz);
    };
    const int N = 4096;
    int jb = -1;
    double best = INFINITY;
    for (int j = 0; j <= N; ++j) {
        const double v = dist(j == N ? a_hi : a_lo + (a_hi - a_lo) * j / N);
        if (v < best) { best = v; jb = j; }
    }
    if (jb < 0) return NAN;
    double lo = a_lo + (a_hi - a_lo) * (jb > 0 ? jb - 1 : 0) / N, hi = a_lo + (a_hi - a_lo) * (jb < N ? jb + 1 : N) / N;
    const double g = 0.5 * (sqrt(5.0) - 1.0);
    for (int it = 0; it < 80; ++it) {
        const double x1 = hi - g * (hi - lo), x2 = lo + g * (hi - lo);
        const double d1 = dist(x1), d2 = dist(x2);
        best = fmin(best, fmin(d1, d2));
        if (d1 < d2) hi = x2; else lo = x1;
    }
    return best;
}

// the radius below which rtus_tt_pipe takes a pipe centred at (x_off, 0): what the geometry fit must stay under
extern "C" double rtus_pipe_clearance(const rtus_lens* lens, double alpha_lo, double alpha_hi, double x_off)
{
    if (!lens || !isfinite(alpha_lo) || !isfinite(alpha_hi) || !(alpha_hi > alpha_lo) || !isfinite(x_off)) return NAN;
    return lens_clearance(*lens, alpha_lo, alpha_hi, x_off);
}

#define RTUS_PIPE_MAX_SCAN 65536
static int check_pipe(const rtus_lens* lens, double a_lo, double a_hi, const rtus_pipe* pipe, double b_lo, double b_hi, int n_scan,
                      const void* xe, const void* ze, int n_e, const void* xf, const void* zf, int n_f, const void* tt)
{
    const int st = check_lens(lens, a_lo, a_hi, xe, ze, n_e > 0 ? 1 : n_e, xf, zf, n_f, tt);   // (the pipe's own limit on n_e is below)
    if (st) return st;
    if (!pipe || !isfinite(lens->c1) || !isfinite(lens->c2)) return RTUS_ERR_INVALID_ARG;
    if (!isfinite(pipe->c3) || !(pipe->c3 > 0) || !isfinite(pipe->r_outer) || !(pipe->r_outer > 0) || !isfinite(pipe->x_off))
        return RTUS_ERR_INVALID_ARG;
    if (!(pipe->r_inner >= 0) || !(pipe->r_inner < pipe->r_outer)) return RTUS_ERR_INVALID_ARG;
    if (!isfinite(b_lo) || !isfinite(b_hi) || !(b_hi > b_lo) || n_scan < 4) return RTUS_ERR_INVALID_ARG;
    if (n_e > 65535 * 8 || n_scan > RTUS_PIPE_MAX_SCAN || (long long)n_e * n_scan > (1LL << 26)) return RTUS_ERR_UNSUPPORTED;
    if (!(pipe->r_outer < lens_clearance(*lens, a_lo, a_hi, pipe->x_off))) return RTUS_ERR_INVALID_ARG;   // touches the lens
    return RTUS_OK;
}

extern "C" size_t rtus_tt_pipe_workspace_bytes(int n_e, int n_scan)
{
    if (n_e <= 0 || n_scan < 4 || n_e > 65535 * 8 || n_scan > RTUS_PIPE_MAX_SCAN || (long long)n_e * n_scan > (1LL << 26)) return 0;
    return rtus_pipe_ws_bytes(n_e, n_scan);
}

extern "C" int rtus_tt_pipe_dev(const rtus_lens* lens, double alpha_lo, double alpha_hi, const rtus_pipe* pipe, double beta_lo,
                                double beta_hi, int n_scan, const double* d_xe, const double* d_ze, int n_e, const double* d_xf,
                                const double* d_zf, int n_f, double* d_tt, double* d_alpha_out, double* d_beta_out, void* d_workspace,
                                size_t workspace_bytes, void* stream)
{
    int st = check_pipe(lens, alpha_lo, alpha_hi, pipe, beta_lo, beta_hi, n_scan, d_xe, d_ze, n_e, d_xf, d_zf, n_f, d_tt);
    if (st) return st;
    if ((st = check_workspace(d_workspace, workspace_bytes, rtus_pipe_ws_bytes(n_e, n_scan), 256))) return st;
    LAUNCH_TRY(rtus_launch_tt_pipe(*lens, alpha_lo, alpha_hi, *pipe, beta_lo, beta_hi, n_scan, d_xe, d_ze, n_e, d_xf, d_zf, n_f, d_tt,
                                   d_alpha_out, d_beta_out, d_workspace, (hipStream_t)stream));
    return RTUS_OK;
}

extern "C" int rtus_tt_pipe(const rtus_lens* lens, double alpha_lo, double alpha_hi, const rtus_pipe* pipe, double beta_lo,
                            double beta_hi, int n_scan, const double* xe, const double* ze, int n_e, const double* xf, const double* zf,
                            int n_f, double* tt, double* alpha_out, double* beta_out, int device)
{
    int st = check_pipe(lens, alpha_lo, alpha_hi, pipe, beta_lo, beta_hi, n_scan, xe, ze, n_e, xf, zf, n_f, tt);
    if (st) return st;
    const size_t tot = (size_t)n_e * n_f;
    Session S;
    if ((st = S.open(device))) return st;
    double *dxe, *dze, *dxf, *dzf, *dtt, *dal, *dbe;
    char* ws;
    S.in(dxe, xe, n_e);
    S.in(dze, ze, n_e);
    S.in(dxf, xf, n_f);
    S.in(dzf, zf, n_f);
    S.out(dtt, tt, tot);
    S.out(dal, alpha_out, tot);
    S.out(dbe, beta_out, tot);
    S.scratch(ws, rtus_pipe_ws_bytes(n_e, n_scan));
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_tt_pipe(*lens, alpha_lo, alpha_hi, *pipe, beta_lo, beta_hi, n_scan, dxe, dze, n_e, dxf, dzf, n_f, dtt, dal, dbe,
                                   ws, S.a->stream));
    return S.finish();
}

// ---------------------------------------------------------------------------- lens -> pipe wall, bore-reflected skip leg
// everything rtus_tt_pipe rejects, a pipe without a bore and a c_up that is not finite and positive
static int check_pipe_skip(const rtus_lens* lens, double a_lo, double a_hi, const rtus_pipe* pipe, double c_up, double b_lo, double b_hi,
                           int n_scan, const void* xe, const void* ze, int n_e, const void* xf, const void* zf, int n_f, const void* tt)
{
    const int st = check_pipe(lens, a_lo, a_hi, pipe, b_lo, b_hi, n_scan, xe, ze, n_e, xf, zf, n_f, tt);
    if (st) return st;
    if (!(pipe->r_inner > 0) || !isfinite(c_up) || !(c_up > 0)) return RTUS_ERR_INVALID_ARG;
    return RTUS_OK;
}

extern "C" size_t rtus_tt_pipe_skip_workspace_bytes(int n_e, int n_scan) { return rtus_tt_pipe_workspace_bytes(n_e, n_scan); }

extern "C" int rtus_tt_pipe_skip_dev(const rtus_lens* lens, double alpha_lo, double alpha_hi, const rtus_pipe* pipe, double c_up,
                                     double beta_lo, double beta_hi, int n_scan, const double* d_xe, const double* d_ze, int n_e,
                                     const double* d_xf, const double* d_zf, int n_f, double* d_tt, double* d_alpha_out, double* d_beta_out,
                                     double* d_gamma_out, void* d_workspace, size_t workspace_bytes, void* stream)
{
    int st = check_pipe_skip(lens, alpha_lo, alpha_hi, pipe, c_up, beta_lo, beta_hi, n_scan, d_xe, d_ze, n_e, d_xf, d_zf, n_f, d_tt);
    if (st) return st;
    if ((st = check_workspace(d_workspace, workspace_bytes, rtus_pipe_ws_bytes(n_e, n_scan), 256))) return st;
    LAUNCH_TRY(rtus_launch_tt_pipe_skip(*lens, alpha_lo, alpha_hi, *pipe, c_up, beta_lo, beta_hi, n_scan, d_xe, d_ze, n_e, d_xf, d_zf, n_f,
                                        d_tt, d_alpha_out, d_beta_out, d_gamma_out, d_workspace, (hipStream_t)stream));
    return RTUS_OK;
}

extern "C" int rtus_tt_pipe_skip(const rtus_lens* lens, double alpha_lo, double alpha_hi, const rtus_pipe* pipe, double c_up, double beta_lo,
                                 double beta_hi, int n_scan, const double* xe, const double* ze, int n_e, const double* xf,
                                 const double* zf, int n_f, double* tt, double* alpha_out, double* beta_out, double* gamma_out, int device)
{
    int st = check_pipe_skip(lens, alpha_lo, alpha_hi, pipe, c_up, beta_lo, beta_hi, n_scan, xe, ze, n_e, xf, zf, n_f, tt);
    if (st) return st;
    const size_t tot = (size_t)n_e * n_f;
    Session S;
    if ((st = S.open(device))) return st;
    double *dxe, *dze, *dxf, *dzf, *dtt, *dal, *dbe, *dga;
    char* ws;
    S.in(dxe, xe, n_e);
    S.in(dze, ze, n_e);
    S.in(dxf, xf, n_f);
    S.in(dzf, zf, n_f);
    S.out(dtt, tt, tot);
    S.out(dal, alpha_out, tot);
    S.out(dbe, beta_out, tot);
    S.out(dga, gamma_out, tot);
    S.scratch(ws, rtus_pipe_ws_bytes(n_e, n_scan));
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_tt_pipe_skip(*lens, alpha_lo, alpha_hi, *pipe, c_up, beta_lo, beta_hi, n_scan, dxe, dze, n_e, dxf, dzf, n_f, dtt,
                                        dal, dbe, dga, ws, S.a->stream));
    return S.finish();
}

// ---------------------------------------------------------------------------- ray amplitude tables of the legs into the pipe wall
static int check_leg_amp_pipe(const rtus_lens* lens, double a_lo, double a_hi, const rtus_pipe* pipe, const rtus_pipe_media* m, int leg,
                              int dir, double width, double f_c, const void* xe, const void* ze, int n_e, const void* xf, const void* zf,
                              int n_f, const void* alpha, const void* beta, const void* gamma, const void* amp)
{
    if (!lens || !pipe || !m || !xe || !ze || !xf || !zf || !alpha || !beta || !amp || n_e <= 0 || n_f <= 0) return RTUS_ERR_INVALID_ARG;
    if (leg < RTUS_LEG_L || leg > RTUS_LEG_TT || (dir != RTUS_AMP_DOWN && dir != RTUS_AMP_UP)) return RTUS_ERR_INVALID_ARG;
    const bool skip = leg >= RTUS_LEG_LL;
    if (skip && !gamma) return RTUS_ERR_INVALID_ARG;
    const double sp[8] = {lens->c1, lens->c2, m->rho_lens, m->ct_lens, m->rho_water, m->rho_wall, m->c_l, m->c_t};
    for (double v : sp)
        if (!isfinite(v) || !(v > 0)) return RTUS_ERR_INVALID_ARG;
    if (!(m->c_t < m->c_l) || !(m->ct_lens < lens->c1) || lens->c1 == lens->c2) return RTUS_ERR_INVALID_ARG;
    if (!isfinite(lens->l0) || !isfinite(lens->h0) || !isfinite(lens->d)) return RTUS_ERR_INVALID_ARG;
    if (!isfinite(pipe->r_outer) || !(pipe->r_outer > 0) || !isfinite(pipe->x_off)) return RTUS_ERR_INVALID_ARG;
    if (!(pipe->r_inner >= 0) || !(pipe->r_inner < pipe->r_outer) || (skip && !(pipe->r_inner > 0))) return RTUS_ERR_INVALID_ARG;
    if (!isfinite(a_lo) || !isfinite(a_hi) || !(a_hi > a_lo)) return RTUS_ERR_INVALID_ARG;
    if (!isfinite(width) || width < 0 || (width > 0 && (!isfinite(f_c) || !(f_c > 0)))) return RTUS_ERR_INVALID_ARG;
    if (n_e > 65535) return RTUS_ERR_UNSUPPORTED;                                         // grid.y: one element per row of workgroups
    return RTUS_OK;
}

extern "C" int rtus_leg_amp_pipe_dev(const rtus_lens* lens, double alpha_lo, double alpha_hi, const rtus_pipe* pipe,
                                     const rtus_pipe_media* media, int leg, int direction, double element_width, double f_c,
                                     const double* d_xe, const double* d_ze, int n_e, const double* d_xf, const double* d_zf, int n_f,
                                     const double* d_alpha, const double* d_beta, const double* d_gamma, float* d_amp, void* stream)
{
    const int st = check_leg_amp_pipe(lens, alpha_lo, alpha_hi, pipe, media, leg, direction, element_width, f_c, d_xe, d_ze, n_e, d_xf,
                                      d_zf, n_f, d_alpha, d_beta, d_gamma, d_amp);
    if (st) return st;
    LAUNCH_TRY(rtus_launch_leg_amp_pipe(*lens, alpha_lo, alpha_hi, *pipe, *media, leg, direction, element_width, f_c, d_xe, d_ze, n_e,
                                        d_xf, d_zf, n_f, d_alpha, d_beta, leg >= RTUS_LEG_LL ? d_gamma : nullptr, d_amp,
                                        (hipStream_t)stream));
    return RTUS_OK;
}

extern "C" int rtus_leg_amp_pipe(const rtus_lens* lens, double alpha_lo, double alpha_hi, const rtus_pipe* pipe,
                                 const rtus_pipe_media* media, int leg, int direction, double element_width, double f_c, const double* xe,
                                 const double* ze, int n_e, const double* xf, const double* zf, int n_f, const double* alpha,
                                 const double* beta, const double* gamma, float* amp, int device)
{
    int st = check_leg_amp_pipe(lens, alpha_lo, alpha_hi, pipe, media, leg, direction, element_width, f_c, xe, ze, n_e, xf, zf, n_f, alpha,
                                beta, gamma, amp);
    if (st) return st;
    const bool skip = leg >= RTUS_LEG_LL;
    const size_t tot = (size_t)n_e * n_f;
    Session S;
    if ((st = S.open(device))) return st;
    double *dxe, *dze, *dxf, *dzf, *dal, *dbe, *dga = nullptr;
    float* damp;
    S.in(dxe, xe, n_e);
    S.in(dze, ze, n_e);
    S.in(dxf, xf, n_f);
    S.in(dzf, zf, n_f);
    S.in(dal, alpha, tot);
    S.in(dbe, beta, tot);
    if (skip) S.in(dga, gamma, tot);
    S.out(damp, amp, 2 * tot);
    if ((st = S.flush())) return st;
    LAUNCH_TRY(rtus_launch_leg_amp_pipe(*lens, alpha_lo, alpha_hi, *pipe, *media, leg, direction, element_width, f_c, dxe, dze, n_e, dxf,
                                        dzf, n_f, dal, dbe, dga, damp, S.a->stream));
    return S.finish();
}
