// Store stream of the planar kernel's row-table path on gfx950, with the build taken out: what do the served rows' stores cost by
// themselves at the headline's shape (BASELINE configs[2]: 256 rows x 262,144 fp64 targets, 537 MB, one launch), and what are the
// store's width, its cache policy, the order of the work items and arithmetic beside the stores each worth?
//   hipcc --offload-arch=gfx950 -O3 scripts/ubench_store_stream.hip -o scripts/ubench_store_stream
//   scripts/ubench_store_stream [rounds, default 15]
// Grid 1024 x 4 workgroups of 256 threads, up to 64 rows per workgroup, launched with the product's LDS (2 KB of records + the
// header, static, and RTUS_ROWTAB_SLOTS x 48 B of table, dynamic) and its launch bounds: eight workgroups per CU.
// Every element gets a value that is an exact function of (row, column); the first launch of every variant is read back and
// compared whole, and a variant that fails is not timed.
//   width   w8     lane <-> one target, every wave writes every row, one 8-byte store per row (512 B per wave-instruction)
//           w16a   a wave serves 128 adjacent targets (lane i: 2 i, 2 i + 1 of its half of the workgroup's 256) and every second
//                  row: waves 0, 1 the even ones, waves 2, 3 the odd ones; one 16-byte store per row (1 KB per wave-instruction)
//           w16h   the same targets; waves 0, 1 take the lower half of the block's rows, waves 2, 3 the upper half
//   policy  the store's cache-policy operand: default (0), nt (2), sc1 (16), sc0 sc1 (17)
//   order   xf: blockIdx.x walks along the rows (neighbouring workgroups write neighbouring 2-KB pieces of the same rows);
//           yf: blockIdx.x walks over the row blocks
//           yflat, rot<k>, rotw<k>, band, b+rot<k>, b+rotw<k>: orders across rows and XCDs on top of w8 sc1 yf (k_order, below)
//   ballast none   stores only
//           serve  per element the served loop's own work: the element's x from LDS, the index, three ds_read_b128 of a 48-byte
//                  slot of the 16.5 KB table, five fp64 FMAs
//           build  serve + a dependent chain of 800 fp64 FMAs per lane before the first store (the table's build, as issue load)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

constexpr int N_F = 262144, N_ROWS = 256, EB = 64, SLOTS = 352;      // RTUS_ROWTAB_SLOTS
struct __attribute__((aligned(16))) Slot { double c[6]; };           // RowTabSlot
struct Rec { float w[4]; double xe; int info, row; };                // ElemRec: 32 bytes
struct Hdr { double v[11]; int i[9]; };                              // RowTabHdr: 124 bytes
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

struct Args { double* out; int n_f, n_rows, eb, yfast; double inv_h, tlo, fa, fb; };

enum { W8 = 0, W16A = 1, W16H = 2 };
enum { NONE = 0, SERVE = 1, BUILD = 2 };

// one served element: (row base + column) exactly, + 0 formed the way the served loop forms T (BAL != NONE)
template <int BAL>
__device__ __forceinline__ double element(double v, double x, double xe, double inv_h, double tlo, const Slot* tab)
{
    if (BAL == NONE) return v;
    const double tq = fma(fabs(x - xe), inv_h, -tlo);
    const double sq = __builtin_amdgcn_fract(tq);
    const Slot* __restrict__ sl = &tab[(int)tq];
    const double T = fma(sq, fma(sq, fma(sq, fma(sq, fma(sq, sl->c[5], sl->c[4]), sl->c[3]), sl->c[2]), sl->c[1]), sl->c[0]);
    return v + (T - (tq - sq));                                       // slot j holds c0 = j, the rest 0: T = floor(tq), exactly
}

template <int W, int AUX, int BAL>
__global__ __launch_bounds__(256, 8) void k_store(Args a)
{
    __shared__ Rec rec[64];
    __shared__ Hdr hdr;
    extern __shared__ __attribute__((aligned(16))) Slot tab[];
    const int bx = a.yfast ? blockIdx.y : blockIdx.x, by = a.yfast ? blockIdx.x : blockIdx.y;
    const int tid = threadIdx.x;
    const int e0 = by * a.eb, ne = min(a.eb, a.n_rows - e0);
    for (int k = tid; k < SLOTS; k += 256) { tab[k].c[0] = (double)k; tab[k].c[1] = tab[k].c[2] = tab[k].c[3] = tab[k].c[4] = tab[k].c[5] = 0.0; }
    if (tid < 64) { rec[tid].xe = -(double)tid; rec[tid].info = 0; }
    if (tid == 0) { hdr.v[0] = a.inv_h; hdr.v[1] = a.tlo; }
    __syncthreads();
    const double inv_h = hdr.v[0], tlo = hdr.v[1];
    double chain = 0.0;
    if (BAL == BUILD) {                                               // 800 dependent fp64 FMAs: fa = 1, fb = 0, unknown to the compiler
        double c = (double)tid;
        for (int t = 0; t < 100; ++t) {
#pragma unroll
            for (int u = 0; u < 8; ++u) c = fma(c, a.fa, a.fb);
        }
        chain = c - (double)tid;                                      // 0
    }
    const unsigned row_bytes = (unsigned)a.n_f * 8u;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(a.out + (size_t)e0 * a.n_f, 0, (unsigned)ne * row_bytes, 0x00020000);
    const double nfd = (double)a.n_f;
    if (W == W8) {
        const int col = bx * 256 + tid;
        const double x = (double)tid + 0.25;                          // the index: tid + l + (0.25 as the fraction)
        double v = (double)e0 * nfd + (double)col + chain;
        unsigned so = 0;
        for (int l = 0; l < ne; ++l) {
            const double T = element<BAL>(v, x, rec[l].xe, inv_h, tlo, tab);
            const u32x2 bits = {(unsigned)__double2loint(T), (unsigned)__double2hiint(T)};
            __builtin_amdgcn_raw_buffer_store_b64(bits, rs, (unsigned)col * 8u, so, AUX);
            v += nfd; so += row_bytes;
        }
    } else {
        const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
        const int c0 = 128 * (w & 1) + 2 * lane, col = bx * 256 + c0;
        const int half = (ne + 1) >> 1;
        const int l0 = W == W16A ? (w >> 1) : ((w >> 1) ? half : 0), l1 = W == W16A ? ne : ((w >> 1) ? ne : half), dl = W == W16A ? 2 : 1;
        const double x0 = (double)c0 + 0.25, x1 = (double)c0 + 1.25;
        double v = (double)(e0 + l0) * nfd + (double)col + chain;
        unsigned so = (unsigned)l0 * row_bytes;
        for (int l = l0; l < l1; l += dl) {
            const double xe = rec[l].xe;
            const double T0 = element<BAL>(v, x0, xe, inv_h, tlo, tab), T1 = element<BAL>(v + 1.0, x1, xe, inv_h, tlo, tab);
            const u32x4 bits = {(unsigned)__double2loint(T0), (unsigned)__double2hiint(T0), (unsigned)__double2loint(T1), (unsigned)__double2hiint(T1)};
            __builtin_amdgcn_raw_buffer_store_b128(bits, rs, (unsigned)col * 8u, so, AUX);
            v += (double)dl * nfd; so += (unsigned)dl * row_bytes;
        }
    }
}

// The adopted shape (w8, sc1, y fastest) with another ORDER of its rows and work items (the table goes to profiles/storestream_order.txt):
//   ROTK   rot(k): the workgroup of column bx serves rows (r0 + i) mod ne, i = 0 .. ne - 1, r0 = (k bx) mod ne — two ranges of one loop
//          body, [r0, ne) then [0, r0) — so workgroups that start together are in different rows (0: every workgroup from row 0)
//   ROTW   rotw(k): wave w adds 16 w to r0 (mod ne): the four waves of a workgroup are in different rows
//   BAND   blockIdx.x = 8 t + x: XCD x (workgroups are dealt round-robin over the eight) takes the columns [x G, (x + 1) G), G = ceil(gx / 8),
//          and walks them y fastest: every XCD sees every row block and both column parities.  The grid is rounded up to 8 G gy;
//          a workgroup past the last column returns before it touches anything.
//   MAP    swz, par, cont<c>: see the kernel
template <int BAL, int ROTK, bool ROTW, bool BAND, int MAP = 0>
__global__ __launch_bounds__(256, 8) void k_order(Args a)
{
    __shared__ Rec rec[64];
    __shared__ Hdr hdr;
    extern __shared__ __attribute__((aligned(16))) Slot tab[];
    const int gx = a.n_f / 256, gy = (a.n_rows + a.eb - 1) / a.eb;
    int bx, by;
    if (BAND) {
        const int x = blockIdx.x & 7, t = blockIdx.x >> 3, G = (gx + 7) / 8;
        by = t % gy; bx = x * G + t / gy;
        if (bx >= gx) return;
    } else { bx = blockIdx.x / gy; by = blockIdx.x % gy; }
    // Permutations of the flat order that keep the window of columns in flight where it is (gy = 4 and gx a multiple of 32, as at the
    // headline: XCD k holds by = k mod 4 and the columns 2 t + k div 4):
    if (MAP == 1) by = (by + (bx >> 1)) % gy;                       // swz: every XCD sees every row block in turn
    if (MAP == 2) bx ^= (bx >> 1) & 1;                              // par: every XCD sees both column parities in turn
    if (MAP >= 4) {                                                 // cont<c>: an XCD's columns come in runs of c = MAP / 2 (flat: 1)
        const int c = MAP / 2, t = bx >> 1, p = bx & 1;
        bx = (t / c) * 2 * c + p * c + t % c;
    }
    const int tid = threadIdx.x;
    const int e0 = by * a.eb, ne = min(a.eb, a.n_rows - e0);
    for (int k = tid; k < SLOTS; k += 256) { tab[k].c[0] = (double)k; tab[k].c[1] = tab[k].c[2] = tab[k].c[3] = tab[k].c[4] = tab[k].c[5] = 0.0; }
    if (tid < 64) { rec[tid].xe = -(double)tid; rec[tid].info = 0; }
    if (tid == 0) { hdr.v[0] = a.inv_h; hdr.v[1] = a.tlo; }
    __syncthreads();
    const double inv_h = hdr.v[0], tlo = hdr.v[1];
    double chain = 0.0;
    if (BAL == BUILD) {
        double c = (double)tid;
        for (int t = 0; t < 100; ++t) {
#pragma unroll
            for (int u = 0; u < 8; ++u) c = fma(c, a.fa, a.fb);
        }
        chain = c - (double)tid;
    }
    const unsigned row_bytes = (unsigned)a.n_f * 8u;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(a.out + (size_t)e0 * a.n_f, 0, (unsigned)ne * row_bytes, 0x00020000);
    const double nfd = (double)a.n_f;
    const int col = bx * 256 + tid;
    const double x = (double)tid + 0.25;
    const double vb = (double)e0 * nfd + (double)col + chain;
    unsigned r0 = (unsigned)ROTK * (unsigned)bx;
    if (ROTW) r0 += 16u * (unsigned)__builtin_amdgcn_readfirstlane(tid >> 6);
    r0 %= (unsigned)ne;
    auto rows = [&](int lo, int hi) {
        double v = vb + (double)lo * nfd;
        unsigned so = (unsigned)lo * row_bytes;
        for (int l = lo; l < hi; ++l) {
            const double T = element<BAL>(v, x, rec[l].xe, inv_h, tlo, tab);
            const u32x2 bits = {(unsigned)__double2loint(T), (unsigned)__double2hiint(T)};
            __builtin_amdgcn_raw_buffer_store_b64(bits, rs, (unsigned)col * 8u, so, 16);
            v += nfd; so += row_bytes;
        }
    };
    rows((int)r0, ne);
    rows(0, (int)r0);
}

struct Variant { char name[48]; void (*fn)(Args); int yfast; std::vector<float> us; bool ok; };

template <int BAL, int ROTK, bool ROTW, bool BAND> static void launch_order(Args a)
{
    const int gx = a.n_f / 256, gy = (a.n_rows + a.eb - 1) / a.eb;
    const unsigned grid = BAND ? 8u * ((gx + 7) / 8) * gy : (unsigned)gx * gy;
    hipLaunchKernelGGL((k_order<BAL, ROTK, ROTW, BAND>), dim3(grid), dim3(256), SLOTS * sizeof(Slot), 0, a);
}

template <int BAL, int ROTK, bool ROTW, bool BAND> static void add_order1(std::vector<Variant>& vs)
{
    static const char* bn[] = {"none", "serve", "build"};
    char on[16];
    if (ROTK) snprintf(on, sizeof on, "%s%s%d", BAND ? "b+" : "", ROTW ? "rotw" : "rot", ROTK);
    else snprintf(on, sizeof on, "%s", BAND ? "band" : "yflat");     // yflat: y fastest through the flattened grid, as the product launches it
    Variant v;
    snprintf(v.name, sizeof v.name, "w8    sc1      %-8s %-6s", on, bn[BAL]);
    v.fn = launch_order<BAL, ROTK, ROTW, BAND>; v.yfast = 1; v.ok = false;
    vs.push_back(v);
}
template <int BAL, int MAP> static void launch_map(Args a)
{
    const int gx = a.n_f / 256, gy = (a.n_rows + a.eb - 1) / a.eb;
    hipLaunchKernelGGL((k_order<BAL, 0, false, false, MAP>), dim3((unsigned)gx * gy), dim3(256), SLOTS * sizeof(Slot), 0, a);
}
template <int BAL, int MAP> static void add_map1(std::vector<Variant>& vs)
{
    static const char* bn[] = {"none", "serve", "build"};
    char on[16];
    if (MAP >= 4) snprintf(on, sizeof on, "cont%d", MAP / 2);
    else snprintf(on, sizeof on, "%s", MAP == 1 ? "swz" : "par");
    Variant v;
    snprintf(v.name, sizeof v.name, "w8    sc1      %-8s %-6s", on, bn[BAL]);
    v.fn = launch_map<BAL, MAP>; v.yfast = 1; v.ok = false;
    vs.push_back(v);
}
template <int MAP> static void add_map(std::vector<Variant>& vs) { add_map1<NONE, MAP>(vs); add_map1<SERVE, MAP>(vs); add_map1<BUILD, MAP>(vs); }
template <int ROTK, bool ROTW, bool BAND> static void add_order(std::vector<Variant>& vs)
{
    add_order1<NONE, ROTK, ROTW, BAND>(vs); add_order1<SERVE, ROTK, ROTW, BAND>(vs); add_order1<BUILD, ROTK, ROTW, BAND>(vs);
}
template <bool BAND> static void add_orders(std::vector<Variant>& vs)
{
    add_order<0, false, BAND>(vs);
    add_order<1, false, BAND>(vs); add_order<4, false, BAND>(vs); add_order<16, false, BAND>(vs);
    add_order<1, true, BAND>(vs); add_order<4, true, BAND>(vs); add_order<16, true, BAND>(vs);
}

template <int W, int AUX, int BAL> static void launch(Args a)
{
    const dim3 grid = a.yfast ? dim3((a.n_rows + a.eb - 1) / a.eb, a.n_f / 256) : dim3(a.n_f / 256, (a.n_rows + a.eb - 1) / a.eb);
    hipLaunchKernelGGL((k_store<W, AUX, BAL>), grid, dim3(256), SLOTS * sizeof(Slot), 0, a);
}

template <int W, int AUX, int BAL> static void add(std::vector<Variant>& vs)
{
    static const char* wn[] = {"w8", "w16a", "w16h"};
    static const char* bn[] = {"none", "serve", "build"};
    const char* pn = AUX == 0 ? "default" : AUX == 2 ? "nt" : AUX == 16 ? "sc1" : "sc0sc1";
    for (int yf = 0; yf < 2; ++yf) {
        Variant v;
        snprintf(v.name, sizeof v.name, "%-5s %-8s %-3s %-6s", wn[W], pn, yf ? "yf" : "xf", bn[BAL]);
        v.fn = launch<W, AUX, BAL>; v.yfast = yf; v.ok = false;
        vs.push_back(v);
    }
}
template <int W, int AUX> static void add_bal(std::vector<Variant>& vs) { add<W, AUX, NONE>(vs); add<W, AUX, SERVE>(vs); add<W, AUX, BUILD>(vs); }
template <int W> static void add_pol(std::vector<Variant>& vs) { add_bal<W, 0>(vs); add_bal<W, 2>(vs); add_bal<W, 16>(vs); add_bal<W, 17>(vs); }

int main(int argc, char** argv)
{
    const int rounds = argc > 1 ? std::max(atoi(argv[1]), 1) : 15, reps = 20;
    const size_t n = (size_t)N_ROWS * N_F, bytes = n * sizeof(double);
    double *dev, *host;
    CHECK(hipMalloc(&dev, bytes));
    CHECK(hipHostMalloc(&host, bytes));
    Args a = {dev, N_F, N_ROWS, EB, 0, 1.0, 0.0, 1.0, 0.0};
    std::vector<Variant> vs;
    add_pol<W8>(vs); add_pol<W16A>(vs); add_pol<W16H>(vs);
    add_orders<false>(vs); add_orders<true>(vs);
    add_map<1>(vs); add_map<2>(vs); add_map<4>(vs); add_map<8>(vs); add_map<32>(vs);

    // every variant once, from a buffer of NaNs (all bits set), compared whole
    for (Variant& v : vs) {
        CHECK(hipMemset(dev, 0xff, bytes));
        a.yfast = v.yfast;
        v.fn(a);
        CHECK(hipGetLastError());
        CHECK(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
        size_t wrong = 0;
        for (size_t i = 0; i < n; ++i) wrong += !(host[i] == (double)i);
        v.ok = wrong == 0;
        if (!v.ok) printf("%s FAILED its compare: %zu of %zu elements wrong; not timed\n", v.name, wrong, n);
    }
    // ~300 ms of untimed launches (an MI355X leaving idle needs a few hundred ms of load to reach the clock it then holds)
    hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    a.yfast = 0;
    for (int i = 0; i < 3000; ++i) vs[0].fn(a);
    CHECK(hipDeviceSynchronize());
    for (int r = 0; r < rounds; ++r)
        for (Variant& v : vs) {
            if (!v.ok) continue;
            a.yfast = v.yfast;
            CHECK(hipEventRecord(e0));
            for (int i = 0; i < reps; ++i) v.fn(a);
            CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1));
            float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
            v.us.push_back(ms / reps * 1e3f);
        }
    printf("%d rows x %d fp64 = %.1f MB per launch; %d rounds of %d back-to-back launches per variant, interleaved\n", N_ROWS, N_F, bytes / 1e6, rounds, reps);
    printf("%-31s %10s %10s %10s %12s\n", "width policy order ballast", "median us", "min us", "max us", "TB/s (med)");
    for (Variant& v : vs) {
        if (!v.ok) continue;
        std::sort(v.us.begin(), v.us.end());
        const float med = v.us[v.us.size() / 2];
        printf("%-31s %10.2f %10.2f %10.2f %12.3f\n", v.name, med, v.us.front(), v.us.back(), bytes / (med * 1e-6) / 1e12);
    }
    CHECK(hipFree(dev)); CHECK(hipHostFree(host));
    return 0;
}
