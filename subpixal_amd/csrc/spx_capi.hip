// libsubpixal_hip.so -- C ABI (include/subpixal_hip.h) over the gfx950 kernels.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC spx_capi.hip
#include "spx_rt_hip.h"
#include "spx_kernels.h"
#include "spx_kernels8.h"
#include "spx_kernels5.h"
#include "spx_kernels128.h"
#include "spx_kernels_big.h"
#include "spx_kernels32.h"
#include "spx_aux_kernels.h"
#include "spx_detect_kernels.h"
#include "spx_error_kernels.h"
#include "spx_drizzle_kernels.h"
#include "spx_drizzle_poly_kernels.h"
#include "spx_crreject_kernels.h"
#include "spx_minmed_kernels.h"
#include "spx_deblend_kernels.h"
#include "spx_background_kernels.h"
#include "spx_sky_kernels.h"
#include "spx_tables.h"
#include "../../include/subpixal_hip.h"

#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#ifndef SPX_DISP5_PACKED_DEFAULT
#define SPX_DISP5_PACKED_DEFAULT 1
#endif
#ifndef SPX_PAIR64_WAVES_DEFAULT
#define SPX_PAIR64_WAVES_DEFAULT 4      // measured: 25.2e6 pairs/s on 4 waves, 18.2e6 on 8 (profiles/r03)
#endif

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int hip_fail(hipError_t e, const char* what) {
    return fail(SPX_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define SPX_HIP(call)                                              \
    do {                                                           \
        hipError_t e__ = (call);                                   \
        if (e__ != hipSuccess) return hip_fail(e__, #call);        \
    } while (0)

// Kernel families (spx_kernels32.h / spx_kernels.h / spx_kernels128.h) and the cutout sides
// they take.  The FFT period is the smallest the path has for which the reference's 'same'
// window (cc.py:114-126) is alias-free: P > 2n - 2 - (n-1)/2.
enum Tile { TILE32 = 0, TILE64 = 1, TILE192 = 2, NUM_TILES = 3, TILE_BIG = 3 };
constexpr int kFoldMaxSide = 85;      // 64 tile, fold path: period 128 covers cutouts up to 85 px
Tile tile_for(int ny, int nx) {
    const int n = ny > nx ? ny : nx;
    return n <= 32 ? TILE32 : (n <= kFoldMaxSide ? TILE64 : (n <= 128 ? TILE192 : TILE_BIG));
}
constexpr int kPeriod[NUM_TILES] = {64, 128, 192};

struct DeviceTables {
    bool ready = false;                          // set only after EVERY table below exists
    spx::cf* tw[NUM_TILES] = {nullptr, nullptr, nullptr};     // w_P^j
    std::map<int, float*> ktab[NUM_TILES];       // upsample -> lane-major interpolation tables
    std::map<int, float*> tw_big;                // general path: class count C -> w_{64C}^j
    std::map<std::pair<int, int>, float*> ktab_big;     // (C, upsample) -> tables
    std::set<const void*> lds_ok;                // kernels whose dynamic-LDS limit is raised
    int num_cu = 256;
    std::mutex launch_mu;                        // serialises enqueues of host threads sharing a device
};

std::mutex g_mu;                                 // guards g_dev and every DeviceTables' maps
std::map<int, DeviceTables> g_dev;

// (float64 tables travel as opaque `float*` device pointers too and are cast back at the launch)
template <typename T> int upload(const std::vector<T>& h, float** out) {
    void* p = nullptr;
    SPX_HIP(hipMalloc(&p, h.size() * sizeof(T)));
    const hipError_t e = hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return hip_fail(e, "hipMemcpy(table)");
    }
    *out = reinterpret_cast<float*>(p);
    return 0;
}

// tables of the calling thread's current device; built on first use.  Everything is built
// into locals and committed together, so a failed allocation leaves no half-initialised state.
int current_tables(DeviceTables** out) {
    int dev = 0;
    SPX_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_mu);
    DeviceTables& t = g_dev[dev];
    if (!t.ready) {
        float* tw[NUM_TILES] = {nullptr, nullptr, nullptr};
        for (int k = 0; k < NUM_TILES; ++k) {
            const int rc = upload(spx::host::make_twiddles(kPeriod[k]), &tw[k]);
            if (rc) {
                for (int j = 0; j < k; ++j) (void)hipFree(tw[j]);
                return rc;
            }
        }
        hipDeviceProp_t prop;
        const hipError_t e = hipGetDeviceProperties(&prop, dev);
        if (e != hipSuccess) {
            for (int j = 0; j < NUM_TILES; ++j) (void)hipFree(tw[j]);
            return hip_fail(e, "hipGetDeviceProperties");
        }
        for (int k = 0; k < NUM_TILES; ++k) t.tw[k] = reinterpret_cast<spx::cf*>(tw[k]);
        t.num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        t.ready = true;
    }
    *out = &t;
    return 0;
}

// Lock order everywhere: g_mu, then a device's launch_mu (spx_shutdown's order).  A launch looks its
// tables up under g_mu, takes launch_mu while still holding it and only then lets g_mu go (TableLock):
// spx_shutdown on another thread therefore cannot free a table between the lookup and the enqueue.
struct TableLock {
    std::unique_lock<std::mutex> g;
    std::unique_lock<std::mutex> launch;
    TableLock() : g(g_mu) {}
    void enter_launch(DeviceTables* t) {
        launch = std::unique_lock<std::mutex>(t->launch_mu);
        g.unlock();
    }
};

// interpolation tables of one tile family for `upsample` (nullptr for upsample 1); caller holds g_mu.
// `f64_64`: the 64 tile's tables as float64 in the float64 MFMA's result order (make_ktab_f64), for the four-wave
// kernel's float64-refine form (PairArgs::refine_f64); the eight-wave A/B kernel always reads float32 ones.
int ktab_for(DeviceTables* t, Tile tile, int upsample, const float** out, bool f64_64 = false) {
    *out = nullptr;
    const int wb = spx::host::window_blocks(upsample);
    if (wb <= 0) return 0;
    f64_64 = f64_64 && tile == TILE64;
    const int key = upsample + (f64_64 ? (1 << 20) : 0);
    auto it = t->ktab[tile].find(key);
    if (it == t->ktab[tile].end()) {
        float* p = nullptr;
        // period 192: float64 tables (its refine stage accumulates in float64)
        const int rc = tile == TILE32 ? upload(spx::host::make_ktab32(upsample, 16 * wb), &p)
                     : tile == TILE64 ? (f64_64 ? upload(spx::host::make_ktab_f64(128, upsample, 16 * wb), &p)
                                                : upload(spx::host::make_ktab(128, upsample, 16 * wb), &p))
                                      : upload(spx::host::make_ktab_big_f64(192, upsample, 16 * wb), &p);
        if (rc) return rc;
        it = t->ktab[tile].emplace(key, p).first;
    }
    *out = it->second;
    return 0;
}
// both forms of a pair-mode launch's tables: `ktab` for the kernel family's refine as this call wants it
// (`refine_f64`: the 64 tile's float64 form), `ktab_f32` for the eight-wave 64-tile kernel (the same pointer
// unless `ktab` is the float64 table)
int pair_tables_for(DeviceTables* t, Tile tile, int upsample, bool refine_f64, const float** ktab,
                    const float** ktab_f32) {
    int rc = ktab_for(t, tile, upsample, ktab, refine_f64);
    if (rc) return rc;
    if (tile == TILE64 && refine_f64) return ktab_for(t, tile, upsample, ktab_f32, false);
    *ktab_f32 = *ktab;
    return 0;
}
// what a call's `refine` argument means for the 64 tile (the other families have one form each: float32 on the
// 32 tile, float64 above 85 px).  The default is float32 at every upsample.  A rule "float64 from three window
// blocks on" was in for an hour of round 3 -- float32 loses 2 % / 10 % of the pairs of sigma 11..15 px spots at
// upsample 39 / 59, float64 none (profiles/r03/width_precision_256.txt) -- until its cost was measured: the
// float64 form takes 12.0 instead of 6.2 ms per 1e5 pairs at upsample 28..43 and 26.3 instead of 11.9 at 59
// (profiles/r03/default_rule_cost.txt: 336 / 512 float64 MFMAs per wave instead of 80; since brought to 8.8 and
// 19.7 ms, f64_live3_ab.txt / f64_live4_ab.txt).  Taking 29..40 % off every such call's rate to cover that corner is
// the caller's decision, not a default: SPX_REFINE_F64.
int refine64_is_f64(int refine, int wb, bool* f64) {
    (void)wb;
    if (refine != SPX_REFINE_DEFAULT && refine != SPX_REFINE_F64 && refine != SPX_REFINE_F32)
        return fail(SPX_E_ARG, "refine must be SPX_REFINE_DEFAULT, SPX_REFINE_F64 or SPX_REFINE_F32");
    *f64 = refine == SPX_REFINE_F64 || (refine == SPX_REFINE_DEFAULT && spx::kRefine64DefaultF64);
    return 0;
}

// general path (cutouts above 128 px): twiddles and tables per class count, built on first use;
// caller holds g_mu
int big_tables_for(DeviceTables* t, int C, int upsample, const spx::cf** tw, const float** ktab) {
    *tw = nullptr;
    *ktab = nullptr;
    auto it = t->tw_big.find(C);
    if (it == t->tw_big.end()) {
        float* p = nullptr;
        const int rc = upload(spx::host::make_twiddles(64 * C), &p);
        if (rc) return rc;
        it = t->tw_big.emplace(C, p).first;
    }
    *tw = reinterpret_cast<const spx::cf*>(it->second);
    const int wb = spx::host::window_blocks(upsample);
    if (wb > 0) {
        auto kt = t->ktab_big.find({C, upsample});
        if (kt == t->ktab_big.end()) {
            float* p = nullptr;
            const int rc = upload(spx::host::make_ktab_big_f64(64 * C, upsample, 16 * wb), &p);
            if (rc) return rc;
            kt = t->ktab_big.emplace(std::make_pair(C, upsample), p).first;
        }
        *ktab = kt->second;
    }
    return 0;
}
// two resident workgroups per CU (as the period-192 path) up to C = 8, one above: the workspace
// of a workgroup is megabytes there (4 C^2 planes + the P x P convolution: 21 MB at C = 16)
int64_t grid_general(int num_cu, int64_t nbatch, int C) {
    const int64_t cap = (int64_t)num_cu * (C <= 8 ? 2 : 1);
    return nbatch < cap ? nbatch : cap;
}

// workgroups of a period-192 launch (each owns one workspace slot)
int64_t grid_big(int num_cu, int64_t nbatch) {
    // SPX_GRID128_PER_CU (tuning knob, default 2): resident workgroups per CU
    static const int per_cu = [] {
        const char* e = getenv("SPX_GRID128_PER_CU");
        const int v = e ? atoi(e) : 2;
        return v >= 1 && v <= 4 ? v : 2;
    }();
    const int64_t cap = (int64_t)num_cu * per_cu;
    return nbatch < cap ? nbatch : cap;
}
int device_cus() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
        return 256;
    return n;
}

// raise a kernel's dynamic-LDS limit: once per kernel instance and device (spx_prepare() does
// it for every instance a later launch can pick, so a captured launch issues no such call)
// (callers hold t->launch_mu)
template <typename K> int allow_lds(DeviceTables* t, K kernel, int bytes) {
    const void* key = reinterpret_cast<const void*>(kernel);
    if (t->lds_ok.count(key)) return 0;
    SPX_HIP(hipFuncSetAttribute(key, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    t->lds_ok.insert(key);
    return 0;
}

// workgroups per launch: enough to fill 256 CUs x 2 resident groups several times
// over; the kernels grid-stride over the batch.
unsigned grid_for(const DeviceTables* t, int64_t nbatch) {
    // SPX_GRID_PER_CU (tuning knob): workgroups launched per CU (2 are resident at a time)
    static const int per_cu = [] {
        const char* e = getenv("SPX_GRID_PER_CU");
        const int v = e ? atoi(e) : 32;
        return v >= 1 && v <= 1024 ? v : 32;
    }();
    const int64_t cap = (int64_t)t->num_cu * per_cu;
    return (unsigned)(nbatch < cap ? nbatch : cap);
}

struct PairArgs {
    int64_t nbatch;
    int ny, nx, U, cc_type;
    const float* ktab;
    const float* ktab_f32;       // for the eight-wave 64-tile kernel (pair_tables_for)
    bool refine_f64;             // 64 tile: the float64-refine form of the four-wave kernel (`ktab` is then float64)
    double* out;
    int32_t* status;
    float* ws;
    hipStream_t s;
};

// One pair-mode kernel instance: `launch` false only raises its LDS limit (spx_prepare).
template <int WB, bool FOLD, typename TIn, int DBG, typename R>
int run_pair64_as(DeviceTables* t, const TIn* ref, const TIn* img, const PairArgs& a, bool launch) {
    const int lds = spx::Lds<2>::total(16 * WB);
    auto kern = spx::pair_kernel<2, WB, DBG, FOLD, TIn, R>;
    int rc = allow_lds(t, kern, lds);
    if (rc || !launch) return rc;
    hipLaunchKernelGGL(kern, dim3(grid_for(t, a.nbatch)), dim3(spx::kThreads), lds, a.s, ref, img,
                       a.nbatch, a.ny, a.nx, a.U, a.cc_type, t->tw[TILE64], a.ktab, a.out, a.status);
    SPX_HIP(hipGetLastError());
    return 0;
}
// The float64-refine form exists for the product instances with a refine stage (DBG = 0, WB > 0); without
// `launch` (spx_prepare) BOTH forms get their LDS limit raised, so either may be launched inside a capture.
template <int WB, bool FOLD, typename TIn, int DBG = 0>
int run_pair64(DeviceTables* t, const TIn* ref, const TIn* img, const PairArgs& a, bool launch) {
    if constexpr (DBG == 0 && WB > 0) {
        if (!launch) {
            const int rc = run_pair64_as<WB, FOLD, TIn, DBG, spx::RefineF64>(t, ref, img, a, false);
            if (rc) return rc;
        } else if (a.refine_f64) {
            return run_pair64_as<WB, FOLD, TIn, DBG, spx::RefineF64>(t, ref, img, a, true);
        }
    }
    return run_pair64_as<WB, FOLD, TIn, DBG, spx::RefineF32>(t, ref, img, a, launch);
}
// the same tile on eight waves per pair (spx_kernels8.h; cutouts up to 64 px, no fold path)
template <int WB, typename TIn, int DBG = 0>
int run_pair64_w8(DeviceTables* t, const TIn* ref, const TIn* img, const PairArgs& a, bool launch) {
    const int lds = spx::w8::L8::total(16 * WB);
    auto kern = spx::w8::pair8_kernel<WB, DBG, TIn>;
    int rc = allow_lds(t, kern, lds);
    if (rc || !launch) return rc;
    hipLaunchKernelGGL(kern, dim3(grid_for(t, a.nbatch)), dim3(spx::w8::kT8), lds, a.s, ref, img,
                       a.nbatch, a.ny, a.nx, a.U, a.cc_type, t->tw[TILE64], a.ktab_f32, a.out, a.status);
    SPX_HIP(hipGetLastError());
    return 0;
}
// SPX_PAIR64_WAVES = 4 | 8 (A/B knob; read once): which kernel takes pair-mode cutouts of 33..64 px
int pair64_waves() {
    static const int w = [] {
        const char* e = getenv("SPX_PAIR64_WAVES");
        const int v = e ? atoi(e) : SPX_PAIR64_WAVES_DEFAULT;
        return v == 4 ? 4 : 8;
    }();
    return w;
}
// 32 tile: one wave per pair, four pairs per workgroup
template <int WB, typename TIn>
int run_pair32(DeviceTables* t, const TIn* ref, const TIn* img, const PairArgs& a, bool launch) {
    const int lds = spx::Lds32::total(16 * (WB > 0 ? WB : 1));
    auto kern = spx::pair32_kernel<WB, TIn>;
    int rc = allow_lds(t, kern, lds);
    if (rc || !launch) return rc;
    hipLaunchKernelGGL(kern, dim3(grid_for(t, (a.nbatch + 3) / 4)), dim3(spx::kThreads), lds, a.s, ref,
                       img, a.nbatch, a.ny, a.nx, a.U, a.cc_type, t->tw[TILE32], a.ktab, a.out, a.status);
    SPX_HIP(hipGetLastError());
    return 0;
}
// period 192 (9 spectral classes, per-workgroup workspace)
template <int WB, typename TIn, int DBG = 0>
int run_pair192(DeviceTables* t, const TIn* ref, const TIn* img, const PairArgs& a, bool launch) {
    const int lds = spx::LdsBig<3>::total(16 * WB);
    auto kern = spx::pair128_kernel<3, WB, DBG, TIn>;
    int rc = allow_lds(t, kern, lds);
    if (rc || !launch) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid_big(t->num_cu, a.nbatch)), dim3(spx::kThreads), lds, a.s,
                       ref, img, a.nbatch, a.ny, a.nx, a.U, a.cc_type, t->tw[TILE192],
                       reinterpret_cast<const double*>(a.ktab), a.out, a.status, a.ws);
    SPX_HIP(hipGetLastError());
    return 0;
}

template <int WB, typename TIn>
int run_pair_wb(DeviceTables* t, Tile tile, bool fold, const TIn* ref, const TIn* img,
                const PairArgs& a, bool launch) {
    switch (tile) {
    case TILE32: return run_pair32<WB, TIn>(t, ref, img, a, launch);
    case TILE64:
        if (fold) return run_pair64<WB, true, TIn>(t, ref, img, a, launch);
        if constexpr (sizeof(TIn) == 4) {      // the eight-wave A/B kernel is built for float32 cutouts only
            if (!launch) {          // spx_prepare: both variants stay launchable inside a capture
                const int rc = run_pair64_w8<WB, TIn>(t, ref, img, a, false);
                return rc ? rc : run_pair64<WB, false, TIn>(t, ref, img, a, false);
            }
            if (pair64_waves() == 8 && !a.refine_f64) return run_pair64_w8<WB, TIn>(t, ref, img, a, true);
        }
        return run_pair64<WB, false, TIn>(t, ref, img, a, launch);
    default: return run_pair192<WB, TIn>(t, ref, img, a, launch);
    }
}
template <typename TIn>
int run_pair(DeviceTables* t, int wb, Tile tile, bool fold, const TIn* ref, const TIn* img,
             const PairArgs& a, bool launch) {
    switch (wb) {
    case 0: return run_pair_wb<0, TIn>(t, tile, fold, ref, img, a, launch);
    case 1: return run_pair_wb<1, TIn>(t, tile, fold, ref, img, a, launch);
    case 2: return run_pair_wb<2, TIn>(t, tile, fold, ref, img, a, launch);
    case 3: return run_pair_wb<3, TIn>(t, tile, fold, ref, img, a, launch);
    default: return run_pair_wb<4, TIn>(t, tile, fold, ref, img, a, launch);
    }
}

struct Disp5Args {
    int64_t nbatch;
    int ny, nx, cc_type;
    float* icc;
    double* out;
    int32_t* status;
    float* ws;
    hipStream_t s;
    spx::ItemTable items;        // per-item offsets and shapes, or nulls for a uniform batch
};
template <typename TIn>
int run_disp5(DeviceTables* t, Tile tile, bool fold, const TIn* ref, const TIn* im4,
              const Disp5Args& a, bool launch) {
    if (tile == TILE192) {
        const int lds = spx::LdsBig<3>::total(0);
        auto kern = spx::disp5_128_kernel<3, TIn>;
        int rc = allow_lds(t, kern, lds);
        if (rc || !launch) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)grid_big(t->num_cu, a.nbatch)), dim3(spx::kThreads), lds,
                           a.s, ref, im4, a.nbatch, a.ny, a.nx, a.cc_type, t->tw[TILE192], a.icc, a.out,
                           a.status, a.ws, a.items);
        SPX_HIP(hipGetLastError());
        return 0;
    }
    if (tile == TILE32) {
        const int lds = spx::Lds32::total(16);
        auto kern = spx::disp5_32_kernel<TIn>;
        int rc = allow_lds(t, kern, lds);
        if (rc || !launch) return rc;
        hipLaunchKernelGGL(kern, dim3(grid_for(t, (a.nbatch + 3) / 4)), dim3(spx::kThreads), lds, a.s, ref,
                           im4, a.nbatch, a.ny, a.nx, a.cc_type, t->tw[TILE32], a.icc, a.out, a.status, a.items);
        SPX_HIP(hipGetLastError());
        return 0;
    }
    // 64 tile: the packed kernel (five transforms per source, one workgroup per CU: spx_kernels5.h) or the
    // round-2 one (eight, two per CU).  Measured on one box, alternating (profiles/r03/disp5_rstd_and_packed_ab.txt,
    // disp5_packed_ab_first.txt): up to 64 px packed is faster for plain CC (+10 %) and NCC (+7 %) and level for
    // ZNCC (-1 %); on the fold path (65..85 px: a staged region twice the size, uncovered on a CU with one
    // workgroup) it is 7-15 % slower.  It takes the cutouts up to 64 px.
    // SPX_DISP5_PACKED = 0 never | 1 that rule (default) | 2 always  (A/B knob, read once)
    static const int mode = [] {
        const char* e = getenv("SPX_DISP5_PACKED");
        const int v = e ? atoi(e) : SPX_DISP5_PACKED_DEFAULT;
        return v < 0 || v > 2 ? 1 : v;
    }();
    const bool packed = mode == 2 || (mode == 1 && !fold);
    {
        const int lds5 = fold ? spx::p5::L5<true>::TOTAL : spx::p5::L5<false>::TOTAL;
        auto k5 = fold ? spx::p5::disp5p_kernel<true, TIn> : spx::p5::disp5p_kernel<false, TIn>;
        int rc5 = allow_lds(t, k5, lds5);
        if (rc5) return rc5;
        if (launch && packed) {
            hipLaunchKernelGGL(k5, dim3(grid_for(t, a.nbatch)), dim3(spx::kThreads), lds5, a.s, ref, im4, a.nbatch,
                               a.ny, a.nx, a.cc_type, t->tw[TILE64], a.icc, a.out, a.status, a.items);
            SPX_HIP(hipGetLastError());
            return 0;
        }
    }
    const int lds = spx::Lds<2>::total(0);
    auto kern = fold ? spx::disp5_kernel<2, true, TIn> : spx::disp5_kernel<2, false, TIn>;
    int rc = allow_lds(t, kern, lds);
    if (rc || !launch) return rc;
    hipLaunchKernelGGL(kern, dim3(grid_for(t, a.nbatch)), dim3(spx::kThreads), lds, a.s, ref, im4, a.nbatch,
                       a.ny, a.nx, a.cc_type, t->tw[TILE64], a.icc, a.out, a.status, a.items);
    SPX_HIP(hipGetLastError());
    return 0;
}

size_t ws_bytes_xcorr(int64_t nbatch, int ny, int nx) {
    if (nbatch <= 0 || ny <= 0 || nx <= 0) return 0;
    const Tile tile = tile_for(ny, nx);
    if (tile == TILE_BIG) {
        const int C = spx::big_class_count(ny, nx);
        return (size_t)grid_general(device_cus(), nbatch, C) * spx::big_ws_floats(C) * sizeof(float);
    }
    if (tile != TILE192) return 0;
    return (size_t)grid_big(device_cus(), nbatch) * spx::kWs96Bytes;
}

template <int WB, typename TIn>
int run_pair_general(DeviceTables* t, const TIn* ref, const TIn* img, const PairArgs& a, int C,
                     const spx::cf* tw, bool launch) {
    const int lds = spx::LdsGen::total(16 * WB);
    auto kern = spx::pair_big_kernel<WB, TIn>;
    int rc = allow_lds(t, kern, lds);
    if (rc || !launch) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid_general(t->num_cu, a.nbatch, C)), dim3(spx::kThreads), lds,
                       a.s, ref, img, a.nbatch, a.ny, a.nx, a.U, a.cc_type, C, tw,
                       reinterpret_cast<const double*>(a.ktab), a.out, a.status, a.ws);
    SPX_HIP(hipGetLastError());
    return 0;
}
template <typename TIn>
int run_pair_general_wb(DeviceTables* t, int wb, const TIn* ref, const TIn* img, const PairArgs& a,
                        int C, const spx::cf* tw, bool launch) {
    switch (wb) {
    case 0: return run_pair_general<0, TIn>(t, ref, img, a, C, tw, launch);
    case 1: return run_pair_general<1, TIn>(t, ref, img, a, C, tw, launch);
    case 2: return run_pair_general<2, TIn>(t, ref, img, a, C, tw, launch);
    case 3: return run_pair_general<3, TIn>(t, ref, img, a, C, tw, launch);
    default: return run_pair_general<4, TIn>(t, ref, img, a, C, tw, launch);
    }
}
template <typename TIn>
int run_disp5_general(DeviceTables* t, const TIn* ref, const TIn* im4, const Disp5Args& a, int C,
                      const spx::cf* tw, bool launch) {
    const int lds = spx::LdsGen::total(0);
    auto kern = spx::disp5_big_kernel<TIn>;
    int rc = allow_lds(t, kern, lds);
    if (rc || !launch) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid_general(t->num_cu, a.nbatch, C)), dim3(spx::kThreads), lds,
                       a.s, ref, im4, a.nbatch, a.ny, a.nx, a.cc_type, C, tw, a.icc, a.out, a.status, a.ws);
    SPX_HIP(hipGetLastError());
    return 0;
}

template <typename TIn>
int xcorr_refine(const TIn* ref, const TIn* img, int64_t nbatch, int ny, int nx, int upsample,
                 int cc_type, int refine, double* out_dxdy, int32_t* out_status, void* workspace,
                 size_t workspace_bytes, void* stream) {
    if (nbatch < 0 || (nbatch > 0 && (!ref || !img || !out_dxdy)))
        return fail(SPX_E_ARG, "null pointer or negative batch");
    bool refine_f64 = false;
    if (int rr = refine64_is_f64(refine, spx::host::window_blocks(upsample), &refine_f64)) return rr;
    if (ny < 5 || nx < 5 || ny > SPX_MAX_SIDE || nx > SPX_MAX_SIDE)
        return fail(SPX_E_SHAPE, "pair mode supports cutouts of 5..682 pixels per side");
    const int wb = spx::host::window_blocks(upsample);
    if (wb < 0) return fail(SPX_E_SHAPE, "upsample must be in [1, 59]");
    if (nbatch == 0) return 0;
    const Tile tile = tile_for(ny, nx);
    if (tile >= TILE192 && (!workspace || workspace_bytes < ws_bytes_xcorr(nbatch, ny, nx)))
        return fail(SPX_E_WORKSPACE, "cutouts above 85 px need spx_workspace_bytes_xcorr() bytes");
    DeviceTables* t = nullptr;
    int rc = current_tables(&t);
    if (rc) return rc;
    PairArgs a = {};
    a.nbatch = nbatch; a.ny = ny; a.nx = nx; a.U = upsample; a.cc_type = cc_type;
    a.out = out_dxdy; a.status = out_status;
    a.ws = reinterpret_cast<float*>(workspace);
    a.s = reinterpret_cast<hipStream_t>(stream);
    TableLock lk;
    if (!t->ready) return fail(SPX_E_ARG, "spx_shutdown() ran between the call's start and its launch");
    if (tile == TILE_BIG) {            // general path: class count and tables at run time
        // Above 128 px the float32 transforms limit the refinement at very fine grids: 11..25-px-wide spots
        // at upsample >= 40 reached 1.2e-3 px against the float64 definition (profiles/r02/sweeps_late.txt),
        // past the 1e-3 px this library promises -- refused rather than returned out of tolerance.
        if (upsample > SPX_MAX_UPSAMPLE_GENERAL)
            return fail(SPX_E_SHAPE, "cutouts above 128 px take upsample 1..39");
        const int C = spx::big_class_count(ny, nx);
        const spx::cf* tw = nullptr;
        rc = big_tables_for(t, C, upsample, &tw, &a.ktab);
        if (rc) return rc;
        lk.enter_launch(t);
        return run_pair_general_wb<TIn>(t, wb, ref, img, a, C, tw, true);
    }
    // the eight-wave A/B kernel has no float64 form: a float64-refine call takes the four-wave kernel
    a.refine_f64 = refine_f64 && tile == TILE64;
    rc = pair_tables_for(t, tile, upsample, a.refine_f64, &a.ktab, &a.ktab_f32);
    if (rc) return rc;
    lk.enter_launch(t);
    return run_pair<TIn>(t, wb, tile, ny > 64 || nx > 64, ref, img, a, true);
}

template <typename TIn>
int find_displacement5(const TIn* ref, const TIn* im4, int64_t nbatch, int ny, int nx, int cc_type,
                       double* out_dxdy, int32_t* out_status, float* out_icc, void* workspace,
                       size_t workspace_bytes, void* stream) {
    if (nbatch < 0 || (nbatch > 0 && (!ref || !im4 || !out_dxdy)))
        return fail(SPX_E_ARG, "null pointer or negative batch");
    if (ny < 3 || nx < 3 || ny > SPX_MAX_SIDE || nx > SPX_MAX_SIDE)
        return fail(SPX_E_SHAPE, "5-image mode supports cutouts of 3..682 pixels per side");
    if (nbatch == 0) return 0;
    const size_t need = spx_workspace_bytes_displacement5(nbatch, ny, nx, out_icc == nullptr);
    if (need > 0 && (!workspace || workspace_bytes < need))
        return fail(SPX_E_WORKSPACE, "workspace missing or smaller than spx_workspace_bytes_displacement5()");
    unsigned char* wsb = reinterpret_cast<unsigned char*>(workspace);
    const size_t tile_ws = ws_bytes_xcorr(nbatch, ny, nx);
    DeviceTables* t = nullptr;
    int rc = current_tables(&t);
    if (rc) return rc;
    Disp5Args a;
    a.items = spx::ItemTable{nullptr, nullptr, 0, 0};
    a.nbatch = nbatch; a.ny = ny; a.nx = nx; a.cc_type = cc_type;
    a.icc = out_icc ? out_icc : reinterpret_cast<float*>(wsb + tile_ws);
    a.out = out_dxdy; a.status = out_status;
    a.ws = reinterpret_cast<float*>(wsb);
    a.s = reinterpret_cast<hipStream_t>(stream);
    TableLock lk;
    if (!t->ready) return fail(SPX_E_ARG, "spx_shutdown() ran between the call's start and its launch");
    if (tile_for(ny, nx) == TILE_BIG) {
        const int C = spx::big_class_count(ny, nx);
        const spx::cf* tw = nullptr;
        const float* unused = nullptr;
        rc = big_tables_for(t, C, 1, &tw, &unused);
        if (rc) return rc;
        lk.enter_launch(t);
        return run_disp5_general<TIn>(t, ref, im4, a, C, tw, true);
    }
    lk.enter_launch(t);
    return run_disp5<TIn>(t, tile_for(ny, nx), ny > 64 || nx > 64, ref, im4, a, true);
}

// reference mode over cutouts of different shapes, all within one kernel family (`family_side`)
template <typename TIn>
int find_displacement5_var(const TIn* ref, const TIn* im4, const int64_t* item_offset,
                           const int32_t* item_shape, int64_t nbatch, int family_side, int cc_type,
                           double* out_dxdy, int32_t* out_status, float* out_icc, void* workspace,
                           size_t workspace_bytes, void* stream) {
    if (nbatch < 0 || (nbatch > 0 && (!ref || !im4 || !item_offset || !item_shape || !out_dxdy || !out_icc)))
        return fail(SPX_E_ARG, "null pointer or negative batch");
    if (family_side < 3 || family_side > 128)
        return fail(SPX_E_SHAPE, "variable-shape batches take cutouts of 3..128 pixels per side");
    if (nbatch == 0) return 0;
    const Tile tile = tile_for(family_side, family_side);
    const size_t need = ws_bytes_xcorr(nbatch, family_side, family_side);
    if (need > 0 && (!workspace || workspace_bytes < need))
        return fail(SPX_E_WORKSPACE, "workspace missing or smaller than spx_workspace_bytes_xcorr()");
    DeviceTables* t = nullptr;
    int rc = current_tables(&t);
    if (rc) return rc;
    const bool fold = family_side > 64;
    Disp5Args a;
    // the largest side the family launched here takes: 32 / 64 / 85 (fold path) / 128
    a.items = spx::ItemTable{item_offset, item_shape,
                             tile == TILE32 ? 32 : (tile == TILE64 ? (fold ? kFoldMaxSide : 64) : 128), 0};
    a.nbatch = nbatch; a.ny = family_side; a.nx = family_side; a.cc_type = cc_type;
    a.icc = out_icc;
    a.out = out_dxdy; a.status = out_status;
    a.ws = reinterpret_cast<float*>(workspace);
    a.s = reinterpret_cast<hipStream_t>(stream);
    TableLock lk;
    if (!t->ready) return fail(SPX_E_ARG, "spx_shutdown() ran between the call's start and its launch");
    lk.enter_launch(t);
    return run_disp5<TIn>(t, tile, fold, ref, im4, a, true);
}

// reference mode over a whole packed catalog: each kernel family named in `family_mask` takes its own items
template <typename TIn>
int find_displacement5_catalog(const TIn* ref, const TIn* im4, const int64_t* item_offset,
                               const int32_t* item_shape, int64_t nbatch, int family_mask, int cc_type,
                               double* out_dxdy, int32_t* out_status, float* out_icc, void* workspace,
                               size_t workspace_bytes, void* stream) {
    if (nbatch < 0 || (nbatch > 0 && (!ref || !im4 || !item_offset || !item_shape || !out_dxdy || !out_icc)))
        return fail(SPX_E_ARG, "null pointer or negative batch");
    if (family_mask & ~15) return fail(SPX_E_ARG, "family_mask has bits 0..3");
    if (nbatch == 0 || family_mask == 0) return 0;
    const size_t need = (family_mask & SPX_FAMILY_128) ? ws_bytes_xcorr(nbatch, 128, 128) : 0;
    if (need > 0 && (!workspace || workspace_bytes < need))
        return fail(SPX_E_WORKSPACE, "workspace missing or smaller than spx_workspace_bytes_xcorr(nbatch, 128, 128)");
    DeviceTables* t = nullptr;
    int rc = current_tables(&t);
    if (rc) return rc;
    // (largest side taken, sides at or below this are another family's, tile, fold path)
    static const struct { int bit, max_side, skip_below; Tile tile; bool fold; } fam[4] = {
        {SPX_FAMILY_32, 32, 2, TILE32, false}, {SPX_FAMILY_64, 64, 32, TILE64, false},
        {SPX_FAMILY_85, kFoldMaxSide, 64, TILE64, true}, {SPX_FAMILY_128, 128, kFoldMaxSide, TILE192, false}};
    TableLock lk;
    if (!t->ready) return fail(SPX_E_ARG, "spx_shutdown() ran between the call's start and its launch");
    lk.enter_launch(t);
    for (int k = 0; k < 4; ++k) {
        if (!(family_mask & fam[k].bit)) continue;
        Disp5Args a;
        a.items = spx::ItemTable{item_offset, item_shape, fam[k].max_side, fam[k].skip_below};
        a.nbatch = nbatch; a.ny = fam[k].max_side; a.nx = fam[k].max_side; a.cc_type = cc_type;
        a.icc = out_icc;
        a.out = out_dxdy; a.status = out_status;
        a.ws = reinterpret_cast<float*>(workspace);
        a.s = reinterpret_cast<hipStream_t>(stream);
        if ((rc = run_disp5<TIn>(t, fam[k].tile, fam[k].fold, ref, im4, a, true))) return rc;
    }
    return 0;
}

// frame -> fixed-shape tiles in the frame's pixel type
template <typename T>
int gather_cutouts(const T* frame, const uint8_t* fmask, int fny, int fnx, const int32_t* boxes, int64_t nbatch,
                   int tny, int tnx, T fill, T* tiles, const int32_t* seg, const int32_t* ids, void* stream) {
    if (nbatch < 0 || (nbatch > 0 && (!frame || !boxes || !tiles)))
        return fail(SPX_E_ARG, "null pointer or negative batch");
    if ((seg == nullptr) != (ids == nullptr))
        return fail(SPX_E_ARG, "seg and ids must be given together");
    if (fny < 1 || fnx < 1 || tny < 1 || tnx < 1) return fail(SPX_E_SHAPE, "bad shape");
    if (nbatch == 0) return 0;
    const int64_t total = nbatch * tny * tnx;
    const int64_t blocks = (total + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 65535 * 32 ? blocks : 65535 * 32);
    hipLaunchKernelGGL(spx::gather_cutouts_kernel<T>, dim3(grid), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), frame, fmask, fny, fnx, boxes, nbatch,
                       tny, tnx, fill, tiles, seg, ids);
    SPX_HIP(hipGetLastError());
    return 0;
}

// frame -> packed variable-shape cutouts in the frame's pixel type
template <typename T>
int gather_cutouts_var(const T* frame, const uint8_t* fmask, int fny, int fnx, const int32_t* boxes,
                       int64_t nbatch, const int64_t* item_offset, T fill, T* packed, const int32_t* seg,
                       const int32_t* ids, void* stream) {
    if (nbatch < 0 || (nbatch > 0 && (!frame || !boxes || !item_offset || !packed)))
        return fail(SPX_E_ARG, "null pointer or negative batch");
    if ((seg == nullptr) != (ids == nullptr))
        return fail(SPX_E_ARG, "seg and ids must be given together");
    if (fny < 1 || fnx < 1) return fail(SPX_E_SHAPE, "bad shape");
    if (nbatch == 0) return 0;
    const unsigned grid = (unsigned)(nbatch < 65535 * 16 ? nbatch : 65535 * 16);
    hipLaunchKernelGGL(spx::gather_cutouts_var_kernel<T>, dim3(grid), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), frame, fmask, fny, fnx, boxes, nbatch,
                       item_offset, fill, packed, seg, ids);
    SPX_HIP(hipGetLastError());
    return 0;
}

// packed drizzled cutouts -> packed blots, stored as TOut (float32 arithmetic either way)
template <typename TOut>
int blot4_var(const float* src, const int64_t* src_offset, const int32_t* src_shape, int64_t nbatch,
              const double* map, int degree, const float* gain, const int64_t* dst_offset,
              const int32_t* dst_shape, TOut* im4, void* stream) {
    if (nbatch < 0 || (nbatch > 0 && (!src || !src_offset || !src_shape || !map || !dst_offset || !dst_shape || !im4)))
        return fail(SPX_E_ARG, "null pointer or negative batch");
    if (degree < 0 || degree > 5) return fail(SPX_E_ARG, "degree: 0 (affine) or 1..5 (polynomial)");
    if (nbatch == 0) return 0;
    const unsigned grid = (unsigned)(nbatch < 65535 * 16 ? nbatch : 65535 * 16);
    hipLaunchKernelGGL(spx::blot4_var_kernel<TOut>, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       src, src_offset, src_shape, nbatch, map, degree, gain, dst_offset, dst_shape, im4);
    SPX_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int spx_abi_version(void) { return SPX_ABI_VERSION; }

const char* spx_last_error(void) { return g_err.c_str(); }

int spx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int spx_init(int device) {
    SPX_HIP(hipSetDevice(device));
    DeviceTables* t = nullptr;
    return current_tables(&t);
}

int spx_prepare(int upsample) {
    const int wb = spx::host::window_blocks(upsample);
    if (wb < 0) return fail(SPX_E_SHAPE, "upsample must be in [1, 59]");
    DeviceTables* t = nullptr;
    int rc = current_tables(&t);
    if (rc) return rc;
    PairArgs pa = {};
    Disp5Args da = {};
    {
        std::lock_guard<std::mutex> gl(g_mu);
        for (int k = 0; k < NUM_TILES; ++k) {
            const float* kt = nullptr;
            const float* kt32 = nullptr;        // both refine forms of the 64 tile: no allocation in a later call
            if ((rc = pair_tables_for(t, (Tile)k, upsample, false, &kt, &kt32))) return rc;
            if ((Tile)k == TILE64 && (rc = pair_tables_for(t, TILE64, upsample, true, &kt, &kt32))) return rc;
        }
    }
    for (int k = 0; k < NUM_TILES; ++k) {
        std::lock_guard<std::mutex> lk(t->launch_mu);
        const Tile tile = (Tile)k;
        for (int fold = 0; fold < (tile == TILE64 ? 2 : 1); ++fold) {
            if ((rc = run_pair<float>(t, wb, tile, fold != 0, nullptr, nullptr, pa, false))) return rc;
            if ((rc = run_pair<double>(t, wb, tile, fold != 0, nullptr, nullptr, pa, false))) return rc;
            if ((rc = run_disp5<float>(t, tile, fold != 0, nullptr, nullptr, da, false))) return rc;
            if ((rc = run_disp5<double>(t, tile, fold != 0, nullptr, nullptr, da, false))) return rc;
        }
    }
    {   // general path (cutouts above 128 px): its tables depend on the cutout size and are built on
        // first use (spx_prepare_shape() builds them up front); the LDS limits are raised here
        std::lock_guard<std::mutex> lk(t->launch_mu);
        if ((rc = run_pair_general_wb<float>(t, wb, nullptr, nullptr, pa, 4, nullptr, false))) return rc;
        if ((rc = run_pair_general_wb<double>(t, wb, nullptr, nullptr, pa, 4, nullptr, false))) return rc;
        if ((rc = run_disp5_general<float>(t, nullptr, nullptr, da, 4, nullptr, false))) return rc;
        if ((rc = run_disp5_general<double>(t, nullptr, nullptr, da, 4, nullptr, false))) return rc;
    }
    return 0;
}

int spx_prepare_shape(int ny, int nx, int upsample) {
    int rc = spx_prepare(upsample);
    if (rc) return rc;
    if (ny < 3 || nx < 3 || ny > SPX_MAX_SIDE || nx > SPX_MAX_SIDE)
        return fail(SPX_E_SHAPE, "cutouts of 3..682 pixels per side");
    if (tile_for(ny, nx) != TILE_BIG) return 0;
    DeviceTables* t = nullptr;
    if ((rc = current_tables(&t))) return rc;
    const spx::cf* tw = nullptr;
    const float* kt = nullptr;
    std::lock_guard<std::mutex> gl(g_mu);
    return big_tables_for(t, spx::big_class_count(ny, nx), upsample, &tw, &kt);
}

int spx_shutdown(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    int prev = 0;
    const bool have_prev = hipGetDevice(&prev) == hipSuccess;
    int rc = 0;
    for (auto& kv : g_dev) {
        DeviceTables& t = kv.second;
        std::lock_guard<std::mutex> ll(t.launch_mu);
        if (hipSetDevice(kv.first) != hipSuccess) { rc = SPX_E_HIP; continue; }
        if (hipDeviceSynchronize() != hipSuccess) rc = SPX_E_HIP;      // no launch may still read a table
        for (int k = 0; k < NUM_TILES; ++k) {
            if (t.tw[k]) (void)hipFree(t.tw[k]);
            t.tw[k] = nullptr;
            for (auto& e : t.ktab[k]) (void)hipFree(e.second);
            t.ktab[k].clear();
        }
        for (auto& e : t.tw_big) (void)hipFree(e.second);
        t.tw_big.clear();
        for (auto& e : t.ktab_big) (void)hipFree(e.second);
        t.ktab_big.clear();
        t.lds_ok.clear();
        t.ready = false;
    }
    if (have_prev) (void)hipSetDevice(prev);
    if (rc) return fail(rc, "spx_shutdown: a device could not be synchronised");
    return 0;
}

size_t spx_workspace_bytes_xcorr(int64_t nbatch, int ny, int nx) { return ws_bytes_xcorr(nbatch, ny, nx); }

// the phase-stamp diagnostic runs on the period-192 path whatever the shape
static size_t workspace_bytes_big(int64_t nbatch) {
    if (nbatch <= 0) return 0;
    return (size_t)grid_big(device_cus(), nbatch) * spx::kWs96Bytes;
}

size_t spx_workspace_bytes_displacement5(int64_t nbatch, int ny, int nx, int need_icc) {
    if (nbatch <= 0 || ny <= 0 || nx <= 0) return 0;
    size_t b = ws_bytes_xcorr(nbatch, ny, nx);
    if (need_icc) b += (size_t)nbatch * 4u * (size_t)ny * (size_t)nx * sizeof(float);
    return b;
}

int spx_xcorr_refine_f32(const float* ref, const float* img, int64_t nbatch, int ny, int nx,
                         int upsample, int cc_type, double* out_dxdy, int32_t* out_status,
                         void* workspace, size_t workspace_bytes, void* stream) {
    return xcorr_refine<float>(ref, img, nbatch, ny, nx, upsample, cc_type, SPX_REFINE_DEFAULT, out_dxdy,
                               out_status, workspace, workspace_bytes, stream);
}
int spx_xcorr_refine_ex_f32(const float* ref, const float* img, int64_t nbatch, int ny, int nx,
                            int upsample, int cc_type, int refine, double* out_dxdy, int32_t* out_status,
                            void* workspace, size_t workspace_bytes, void* stream) {
    return xcorr_refine<float>(ref, img, nbatch, ny, nx, upsample, cc_type, refine, out_dxdy, out_status,
                               workspace, workspace_bytes, stream);
}
int spx_xcorr_refine_f64(const double* ref, const double* img, int64_t nbatch, int ny, int nx,
                         int upsample, int cc_type, double* out_dxdy, int32_t* out_status,
                         void* workspace, size_t workspace_bytes, void* stream) {
    return xcorr_refine<double>(ref, img, nbatch, ny, nx, upsample, cc_type, SPX_REFINE_DEFAULT, out_dxdy,
                                out_status, workspace, workspace_bytes, stream);
}
int spx_xcorr_refine_ex_f64(const double* ref, const double* img, int64_t nbatch, int ny, int nx,
                            int upsample, int cc_type, int refine, double* out_dxdy, int32_t* out_status,
                            void* workspace, size_t workspace_bytes, void* stream) {
    return xcorr_refine<double>(ref, img, nbatch, ny, nx, upsample, cc_type, refine, out_dxdy, out_status,
                                workspace, workspace_bytes, stream);
}

#ifdef SPX_PHASE_TIMING
// Diagnostic library only (`make diag`): the pair kernel (upsample 10) cut short after
// phase `phase` (1..13, see tools/phase_timing.py); results are invalid.  phase 100 =
// full kernel with per-phase cycle stamps: out_status must have room for nbatch int32
// + 20 uint64 (8-byte aligned: nbatch even), zeroed by the caller.
int spx_diag_pair_phase(const float* ref, const float* img, int64_t nbatch, int ny, int nx,
                        int phase, double* out_dxdy, int32_t* out_status, void* stream) {
    DeviceTables* t = nullptr;
    int rc = current_tables(&t);
    if (rc) return rc;
    PairArgs a = {};
    a.nbatch = nbatch; a.ny = ny; a.nx = nx; a.U = 10; a.cc_type = 0; a.out = out_dxdy;
    a.status = out_status; a.ws = nullptr; a.s = reinterpret_cast<hipStream_t>(stream);
    {
        std::lock_guard<std::mutex> gl(g_mu);
        a.refine_f64 = false;
        rc = pair_tables_for(t, TILE64, 10, false, &a.ktab, &a.ktab_f32);
    }
    if (rc) return rc;
    const bool fold = ny > 64 || nx > 64;
#define SPX_PH(k) case k: return fold ? run_pair64<1, true, float, k>(t, ref, img, a, true) \
                                      : run_pair64<1, false, float, k>(t, ref, img, a, true);
    // phases 200 + k: the eight-wave kernel (k = 1 staging only, 10 through the planes, 100 stamps)
    if (phase == 201) return run_pair64_w8<1, float, 1>(t, ref, img, a, true);
    if (phase == 210) return run_pair64_w8<1, float, 10>(t, ref, img, a, true);
    if (phase == 300) return run_pair64_w8<1, float, 100>(t, ref, img, a, true);
    switch (phase) {
        SPX_PH(0) SPX_PH(1) SPX_PH(2) SPX_PH(3) SPX_PH(4) SPX_PH(5) SPX_PH(6) SPX_PH(7)
        SPX_PH(8) SPX_PH(9) SPX_PH(10) SPX_PH(11) SPX_PH(12) SPX_PH(13) SPX_PH(100)
    }
#undef SPX_PH
    return fail(SPX_E_ARG, "bad phase");
}

// same for the period-192 path at upsample 20 (full kernel with per-phase stamps only)
int spx_diag_pair128_phase(const float* ref, const float* img, int64_t nbatch, int ny, int nx,
                           double* out_dxdy, int32_t* out_status, void* workspace,
                           size_t workspace_bytes, void* stream) {
    DeviceTables* t = nullptr;
    int rc = current_tables(&t);
    if (rc) return rc;
    if (workspace_bytes < workspace_bytes_big(nbatch)) return fail(SPX_E_WORKSPACE, "workspace");
    PairArgs a = {};
    a.nbatch = nbatch; a.ny = ny; a.nx = nx; a.U = 20; a.cc_type = 0; a.out = out_dxdy;
    a.status = out_status; a.ws = reinterpret_cast<float*>(workspace);
    a.s = reinterpret_cast<hipStream_t>(stream);
    {
        std::lock_guard<std::mutex> gl(g_mu);
        rc = ktab_for(t, TILE192, 20, &a.ktab);
    }
    if (rc) return rc;
    return run_pair192<2, float, 100>(t, ref, img, a, true);
}
size_t spx_diag_workspace_bytes_big(int64_t nbatch) { return workspace_bytes_big(nbatch); }
#endif

int spx_find_displacement5_f32(const float* ref, const float* im4, int64_t nbatch, int ny,
                               int nx, int cc_type, double* out_dxdy, int32_t* out_status,
                               float* out_icc, void* workspace, size_t workspace_bytes,
                               void* stream) {
    return find_displacement5<float>(ref, im4, nbatch, ny, nx, cc_type, out_dxdy, out_status, out_icc,
                                     workspace, workspace_bytes, stream);
}
int spx_find_displacement5_f64(const double* ref, const double* im4, int64_t nbatch, int ny,
                               int nx, int cc_type, double* out_dxdy, int32_t* out_status,
                               float* out_icc, void* workspace, size_t workspace_bytes,
                               void* stream) {
    return find_displacement5<double>(ref, im4, nbatch, ny, nx, cc_type, out_dxdy, out_status, out_icc,
                                      workspace, workspace_bytes, stream);
}

int spx_find_displacement5_var_f32(const float* ref, const float* im4, const int64_t* item_offset,
                                   const int32_t* item_shape, int64_t nbatch, int family_side,
                                   int cc_type, double* out_dxdy, int32_t* out_status, float* out_icc,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    return find_displacement5_var<float>(ref, im4, item_offset, item_shape, nbatch, family_side, cc_type,
                                         out_dxdy, out_status, out_icc, workspace, workspace_bytes, stream);
}
int spx_find_displacement5_var_f64(const double* ref, const double* im4, const int64_t* item_offset,
                                   const int32_t* item_shape, int64_t nbatch, int family_side,
                                   int cc_type, double* out_dxdy, int32_t* out_status, float* out_icc,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    return find_displacement5_var<double>(ref, im4, item_offset, item_shape, nbatch, family_side, cc_type,
                                          out_dxdy, out_status, out_icc, workspace, workspace_bytes, stream);
}

int spx_find_displacement5_catalog_f32(const float* ref, const float* im4, const int64_t* item_offset,
                                       const int32_t* item_shape, int64_t nbatch, int family_mask,
                                       int cc_type, double* out_dxdy, int32_t* out_status,
                                       float* out_icc, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    return find_displacement5_catalog<float>(ref, im4, item_offset, item_shape, nbatch, family_mask, cc_type,
                                             out_dxdy, out_status, out_icc, workspace, workspace_bytes, stream);
}
int spx_find_displacement5_catalog_f64(const double* ref, const double* im4, const int64_t* item_offset,
                                       const int32_t* item_shape, int64_t nbatch, int family_mask,
                                       int cc_type, double* out_dxdy, int32_t* out_status,
                                       float* out_icc, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    return find_displacement5_catalog<double>(ref, im4, item_offset, item_shape, nbatch, family_mask, cc_type,
                                              out_dxdy, out_status, out_icc, workspace, workspace_bytes, stream);
}

int spx_gather_cutouts_var_f32(const float* frame, const uint8_t* fmask, int fny, int fnx,
                               const int32_t* boxes, int64_t nbatch, const int64_t* item_offset,
                               float fill, float* packed, const int32_t* seg, const int32_t* ids,
                               void* stream) {
    return gather_cutouts_var<float>(frame, fmask, fny, fnx, boxes, nbatch, item_offset, fill, packed, seg, ids,
                                     stream);
}
int spx_gather_cutouts_var_f64(const double* frame, const uint8_t* fmask, int fny, int fnx,
                               const int32_t* boxes, int64_t nbatch, const int64_t* item_offset,
                               double fill, double* packed, const int32_t* seg, const int32_t* ids,
                               void* stream) {
    return gather_cutouts_var<double>(frame, fmask, fny, fnx, boxes, nbatch, item_offset, fill, packed, seg, ids,
                                      stream);
}

int spx_blot4_var_f32(const float* src, const int64_t* src_offset, const int32_t* src_shape,
                      int64_t nbatch, const double* map, int degree, const float* gain,
                      const int64_t* dst_offset, const int32_t* dst_shape, float* im4, void* stream) {
    return blot4_var<float>(src, src_offset, src_shape, nbatch, map, degree, gain, dst_offset, dst_shape, im4,
                            stream);
}
int spx_blot4_var_to_f64(const float* src, const int64_t* src_offset, const int32_t* src_shape,
                         int64_t nbatch, const double* map, int degree, const float* gain,
                         const int64_t* dst_offset, const int32_t* dst_shape, double* im4, void* stream) {
    return blot4_var<double>(src, src_offset, src_shape, nbatch, map, degree, gain, dst_offset, dst_shape, im4,
                             stream);
}

int spx_find_peak_f64(const double* image, const uint8_t* mask, const double* guess,
                      int64_t nbatch, int ny, int nx, int fit_wx, int fit_wy, int search_wx,
                      int search_wy, double* out_xy, int32_t* out_status, void* stream) {
    if (nbatch < 0 || (nbatch > 0 && (!image || !out_xy)))
        return fail(SPX_E_ARG, "null pointer or negative batch");
    if (ny < 1 || nx < 1 || (int64_t)ny * nx > (int64_t)1 << 30)
        return fail(SPX_E_SHAPE, "bad image shape");
    if (fit_wx < 1 || fit_wy < 1 || search_wx < 0 || search_wy < 0 ||
        ((search_wx == 0) != (search_wy == 0)))
        return fail(SPX_E_ARG, "box dimensions must be positive (search box: both 0 = off)");
    if ((int64_t)fit_wx * fit_wy > spx::kPeakMaxFitPoints)
        return fail(SPX_E_SHAPE, "fit box larger than 1024 points");
    if (nbatch == 0) return 0;
    const unsigned grid = (unsigned)(nbatch < 65535 * 16 ? nbatch : 65535 * 16);
    hipLaunchKernelGGL(spx::find_peak_kernel, dim3(grid), dim3(spx::kThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), image, mask, guess, nbatch, ny, nx,
                       fit_wx, fit_wy, search_wx, search_wy, out_xy, out_status);
    SPX_HIP(hipGetLastError());
    return 0;
}

int spx_gather_cutouts_f32(const float* frame, const uint8_t* fmask, int fny, int fnx,
                           const int32_t* boxes, int64_t nbatch, int tny, int tnx, float fill,
                           float* tiles, const int32_t* seg, const int32_t* ids, void* stream) {
    return gather_cutouts<float>(frame, fmask, fny, fnx, boxes, nbatch, tny, tnx, fill, tiles, seg, ids, stream);
}
int spx_gather_cutouts_f64(const double* frame, const uint8_t* fmask, int fny, int fnx,
                           const int32_t* boxes, int64_t nbatch, int tny, int tnx, double fill,
                           double* tiles, const int32_t* seg, const int32_t* ids, void* stream) {
    return gather_cutouts<double>(frame, fmask, fny, fnx, boxes, nbatch, tny, tnx, fill, tiles, seg, ids, stream);
}

int spx_label_bboxes_i32(const int32_t* seg, int fny, int fnx, int32_t max_label,
                         int32_t* boxes, int32_t* counts, void* stream) {
    if (!seg || !boxes || !counts) return fail(SPX_E_ARG, "null pointer");
    if (fny < 1 || fnx < 1 || max_label < 0) return fail(SPX_E_SHAPE, "bad shape");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int nl = max_label + 1;
    hipLaunchKernelGGL(spx::label_bbox_init_kernel, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, s,
                       boxes, counts, nl);
    SPX_HIP(hipGetLastError());
    const int64_t total = (int64_t)fny * ((fnx + 3) / 4);
    const int64_t blocks = (total + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 8192 ? blocks : 8192);
    hipLaunchKernelGGL(spx::label_bbox_kernel, dim3(grid), dim3(256), 0, s, seg, fny, fnx,
                       (int)max_label, boxes, counts);
    SPX_HIP(hipGetLastError());
    return 0;
}

int spx_blot_affine4_f32(const float* src, int64_t nbatch, int sny, int snx, const double* affine,
                         const float* gain, int ny, int nx, float* im4, void* stream) {
    if (nbatch < 0 || (nbatch > 0 && (!src || !affine || !im4)))
        return fail(SPX_E_ARG, "null pointer or negative batch");
    if (sny < 6 || snx < 6 || sny > 4096 || snx > 4096 || ny < 1 || nx < 1 || ny > 4096 || nx > 4096)
        return fail(SPX_E_SHAPE, "source tiles must be 6..4096 px per side, targets 1..4096");
    if (nbatch == 0) return 0;
    const int64_t total = nbatch * 4 * ny * nx;
    const int64_t blocks = (total + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 65536 ? blocks : 65536);
    hipLaunchKernelGGL(spx::blot_affine4_kernel, dim3(grid), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), src, nbatch, sny, snx, affine, gain, ny,
                       nx, im4);
    SPX_HIP(hipGetLastError());
    return 0;
}

int spx_blot_poly4_f32(const float* src, int64_t nbatch, int sny, int snx, const double* coef,
                       int degree, const float* gain, int ny, int nx, float* im4, void* stream) {
    if (nbatch < 0 || (nbatch > 0 && (!src || !coef || !im4)))
        return fail(SPX_E_ARG, "null pointer or negative batch");
    if (degree < 1 || degree > 5) return fail(SPX_E_ARG, "polynomial degree must be 1..5");
    if (sny < 6 || snx < 6 || sny > 4096 || snx > 4096 || ny < 1 || nx < 1 || ny > 4096 || nx > 4096)
        return fail(SPX_E_SHAPE, "source tiles must be 6..4096 px per side, targets 1..4096");
    if (nbatch == 0) return 0;
    const int64_t total = nbatch * 4 * ny * nx;
    const int64_t blocks = (total + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 65536 ? blocks : 65536);
    hipLaunchKernelGGL(spx::blot_poly4_kernel, dim3(grid), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), src, nbatch, sny, snx, coef, degree, gain,
                       ny, nx, im4);
    SPX_HIP(hipGetLastError());
    return 0;
}

int spx_gen_gaussian_pairs_f32(uint64_t seed, int64_t first_index, int64_t nbatch, int n,
                               float sigma_lo, float sigma_hi, float max_shift, float* ref,
                               float* img, double* truth_dxdy, void* stream) {
    if (nbatch < 0 || (nbatch > 0 && (!ref || !img)))
        return fail(SPX_E_ARG, "null pointer or negative batch");
    if (n < 1 || n > 4096) return fail(SPX_E_SHAPE, "bad tile size");
    if (nbatch == 0) return 0;
    const unsigned grid = (unsigned)(nbatch < 65535 * 16 ? nbatch : 65535 * 16);
    hipLaunchKernelGGL(spx::gen_pairs_kernel, dim3(grid), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), seed, first_index, nbatch, n, sigma_lo,
                       sigma_hi, max_shift, ref, img, truth_dxdy);
    SPX_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------
// source finding (spx_detect_kernels.h).  Workspace: R int32 [npix] | cnt int32 [npix] | chunk sums int32
// [ceil(npix / 1024)] | status int32, each part on a 256-byte boundary.
// ---------------------------------------------------------------------------------------------------------
namespace {
struct DetectLayout {
    size_t r, cnt, sums, status, total;
};
DetectLayout detect_layout(int64_t npix) {
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    DetectLayout d;
    d.r = 0;
    d.cnt = up((size_t)npix * 4);
    d.sums = d.cnt + up((size_t)npix * 4);
    d.status = d.sums + up((size_t)((npix + spx::kDetChunk - 1) / spx::kDetChunk) * 4);
    d.total = d.status + 256;
    return d;
}
unsigned capped_grid(int64_t blocks, int64_t cap = 65536) {
    return (unsigned)(blocks < 1 ? 1 : (blocks < cap ? blocks : cap));
}

template <typename T>
int detect_label(const T* frame, const uint8_t* bad, T thr_scalar, const float* thr_map, const T* filter, int fky,
                 int fkx, int fny, int fnx, int conn, int min_area, void* work, size_t work_bytes,
                 int32_t* out_labels, int32_t* out_nlabels, void* stream) {
    if (!frame || !out_labels || !out_nlabels) return fail(SPX_E_ARG, "null pointer");
    if (fny < 1 || fnx < 1 || (int64_t)fny * fnx >= 2147483647LL)
        return fail(SPX_E_SHAPE, "the frame must hold 1 .. 2^31 - 2 pixels");
    if (conn != 4 && conn != 8) return fail(SPX_E_ARG, "connectivity must be 4 or 8");
    if (min_area < 1) return fail(SPX_E_ARG, "min_area must be at least 1");
    if (!filter) fky = fkx = 1;
    if (fky < 1 || fkx < 1 || !(fky & 1) || !(fkx & 1) || fky > spx::kDetMaxFilter || fkx > spx::kDetMaxFilter)
        return fail(SPX_E_ARG, "filter sides must be odd and at most 7");
    const int npix = fny * fnx;
    const DetectLayout lay = detect_layout(npix);
    if (!work || work_bytes < lay.total)
        return fail(SPX_E_WORKSPACE, "workspace missing or smaller than spx_detect_workspace_bytes(fny, fnx)");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* w = static_cast<char*>(work);
    int32_t* R = reinterpret_cast<int32_t*>(w + lay.r);
    int32_t* cnt = reinterpret_cast<int32_t*>(w + lay.cnt);
    int32_t* sums = reinterpret_cast<int32_t*>(w + lay.sums);
    int32_t* status = reinterpret_cast<int32_t*>(w + lay.status);
    SPX_HIP(hipMemsetAsync(status, 0, 4, s));
    const int64_t ntiles = (int64_t)((fnx + spx::kDetTW - 1) / spx::kDetTW) * ((fny + spx::kDetTH - 1) / spx::kDetTH);
    hipLaunchKernelGGL(spx::detect_tile_kernel<T>, dim3(capped_grid(ntiles, 1 << 20)), dim3(256),
                       spx::det_tile_lds_bytes(sizeof(T), fky, fkx), s, frame, bad, thr_scalar, thr_map, filter,
                       fky, fkx, fny, fnx, conn, out_labels, cnt, status);
    SPX_HIP(hipGetLastError());
    const int64_t nborder = (int64_t)((fny + spx::kDetTH - 1) / spx::kDetTH - 1) * fnx +
                            2 * (int64_t)((fnx + spx::kDetTW - 1) / spx::kDetTW - 1) * fny;
    if (nborder > 0) {
        hipLaunchKernelGGL(spx::detect_border_kernel, dim3(capped_grid((nborder + 255) / 256)), dim3(256), 0, s,
                           out_labels, fny, fnx, conn, status);
        SPX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(spx::detect_compress_kernel, dim3(capped_grid(((int64_t)npix + 1023) / 1024)), dim3(256), 0,
                       s, out_labels, npix, R, cnt, status);
    SPX_HIP(hipGetLastError());
    const int64_t nchunks = ((int64_t)npix + spx::kDetChunk - 1) / spx::kDetChunk;
    hipLaunchKernelGGL(spx::detect_flag_count_kernel, dim3(capped_grid(nchunks)), dim3(256), spx::kDetScanLdsBytes,
                       s, R, cnt, npix, min_area, sums);
    SPX_HIP(hipGetLastError());
    hipLaunchKernelGGL(spx::detect_scan_blocks_kernel, dim3(1), dim3(256), spx::kDetScanLdsBytes, s, sums, nchunks,
                       status, out_nlabels);
    SPX_HIP(hipGetLastError());
    hipLaunchKernelGGL(spx::detect_assign_kernel, dim3(capped_grid(nchunks)), dim3(256), spx::kDetScanLdsBytes, s,
                       R, cnt, npix, min_area, sums);
    SPX_HIP(hipGetLastError());
    hipLaunchKernelGGL(spx::detect_relabel_kernel, dim3(capped_grid(((int64_t)npix + 255) / 256)), dim3(256), 0, s,
                       R, cnt, npix, out_labels);
    SPX_HIP(hipGetLastError());
    return 0;
}

template <typename T>
int measure_labels(const T* frame, const uint8_t* bad, double bkg_scalar, const T* bkg_map, const int32_t* labels,
                   int fny, int fnx, int nlabels, const int32_t* boxes, double* table, int32_t* flags,
                   void* stream) {
    if (nlabels < 0) return fail(SPX_E_ARG, "negative label count");
    if (fny < 1 || fnx < 1 || (int64_t)fny * fnx >= 2147483647LL)
        return fail(SPX_E_SHAPE, "the frame must hold 1 .. 2^31 - 2 pixels");
    if (nlabels == 0) return 0;
    if (!frame || !labels || !boxes || !table || !flags) return fail(SPX_E_ARG, "null pointer");
    hipLaunchKernelGGL(spx::measure_labels_kernel<T>, dim3(capped_grid(nlabels, 1 << 20)), dim3(256),
                       spx::kMeasureLdsBytes, reinterpret_cast<hipStream_t>(stream), frame, bad, bkg_scalar, bkg_map,
                       labels, fny, fnx, nlabels, boxes, table, flags);
    SPX_HIP(hipGetLastError());
    return 0;
}

template <typename T>
int measure_errors(const T* frame, const uint8_t* bad, double bkg_scalar, const T* bkg_map, double rms_scalar,
                   const T* rms_map, double gain, const int32_t* labels, int fny, int fnx, int nlabels,
                   const int32_t* boxes, const double* table, double* out, int32_t* out_flags, void* stream) {
    if (nlabels < 0) return fail(SPX_E_ARG, "negative label count");
    if (fny < 1 || fnx < 1 || (int64_t)fny * fnx >= 2147483647LL)
        return fail(SPX_E_SHAPE, "the frame must hold 1 .. 2^31 - 2 pixels");
    if (nlabels == 0) return 0;
    if (!frame || !labels || !boxes || !table || !out || !out_flags) return fail(SPX_E_ARG, "null pointer");
    hipLaunchKernelGGL(spx::measure_errors_kernel<T>, dim3(capped_grid(nlabels, 1 << 20)), dim3(256),
                       spx::kErrorLdsBytes, reinterpret_cast<hipStream_t>(stream), frame, bad, bkg_scalar, bkg_map,
                       rms_scalar, rms_map, gain, labels, fny, fnx, nlabels, boxes, table, out, out_flags);
    SPX_HIP(hipGetLastError());
    return 0;
}

static_assert(sizeof(spx::DrizzleRow) == SPX_DRIZZLE_ROW_BYTES, "include/subpixal_hip.h states the row size");
int drizzle_sizes(int nframes, int kernel, int out_ny, int out_nx) {
    if (nframes < 1 || nframes > spx::kDrzMaxFrames) return fail(SPX_E_ARG, "nframes must be 1..128");
    if (kernel < 0 || kernel > 2) return fail(SPX_E_ARG, "kernel must be 0 (square), 1 (turbo) or 2 (point)");
    if (out_ny < 1 || out_nx < 1 || (int64_t)out_ny * out_nx >= 2147483647LL)
        return fail(SPX_E_SHAPE, "the output must hold 1 .. 2^31 - 2 pixels");
    return 0;
}

template <typename T>
int drizzle(const void* rows, int nframes, int kernel, double fill, int out_ny, int out_nx, T* sci, float* wht,
            int32_t* ctx, void* stream) {
    if (const int rc = drizzle_sizes(nframes, kernel, out_ny, out_nx)) return rc;
    if (!rows || !sci || !wht || !ctx) return fail(SPX_E_ARG, "null pointer");
    const int64_t tiles = (int64_t)((out_nx + spx::kDrzTileW - 1) / spx::kDrzTileW) *
                          ((out_ny + spx::kDrzTileH - 1) / spx::kDrzTileH);
    hipLaunchKernelGGL(spx::drizzle_kernel<T>, dim3(capped_grid(tiles, 1 << 20)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), static_cast<const spx::DrizzleRow*>(rows), nframes,
                       kernel, fill, out_ny, out_nx, sci, wht, ctx);
    SPX_HIP(hipGetLastError());
    return 0;
}

static_assert(sizeof(spx::DrizzlePolyRow) == SPX_DRIZZLE_POLY_ROW_BYTES, "include/subpixal_hip.h states the row size");
// (subpixal_amd/_ffi.py names these offsets for the tools and tests that read a packed row)
static_assert(offsetof(spx::DrizzlePolyRow, coef) == 40 && offsetof(spx::DrizzlePolyRow, xc) == 376 &&
                  offsetof(spx::DrizzlePolyRow, inv) == 392 && offsetof(spx::DrizzlePolyRow, rx) == 424 &&
                  offsetof(spx::DrizzlePolyRow, bx) == 456 && offsetof(spx::DrizzlePolyRow, degree) == 480,
              "subpixal_amd/_ffi.py states the field offsets");
template <typename T>
int drizzle_poly(const void* rows, int nframes, int kernel, double fill, int out_ny, int out_nx, T* sci, float* wht,
                 int32_t* ctx, void* stream) {
    if (const int rc = drizzle_sizes(nframes, kernel, out_ny, out_nx)) return rc;
    if (!rows || !sci || !wht || !ctx) return fail(SPX_E_ARG, "null pointer");
    const int64_t tiles = (int64_t)((out_nx + spx::kDrzTileW - 1) / spx::kDrzTileW) *
                          ((out_ny + spx::kDrzTileH - 1) / spx::kDrzTileH);
    hipLaunchKernelGGL(spx::drizzle_poly_kernel<T>, dim3(capped_grid(tiles, 1 << 20)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), static_cast<const spx::DrizzlePolyRow*>(rows), nframes,
                       kernel, fill, out_ny, out_nx, sci, wht, ctx);
    SPX_HIP(hipGetLastError());
    return 0;
}

// cosmic-ray rejection (spx_crreject_kernels.h)
std::mutex g_crr_mu;
std::set<std::pair<int, const void*>> g_crr_lds_ok;       // (device, kernel) whose dynamic-LDS limit is raised

template <typename T>
int drizzle_median(const void* rows, int nframes, int nactive, int kernel, int nlow, int nhigh, int out_ny, int out_nx,
                   float* med, uint8_t* nmed, void* stream) {
    if (const int rc = drizzle_sizes(nframes, kernel, out_ny, out_nx)) return rc;
    if (nactive < 1 || nactive > nframes) return fail(SPX_E_ARG, "nactive must be 1..nframes");
    if (nlow < 0 || nhigh < 0) return fail(SPX_E_ARG, "nlow and nhigh must not be negative");
    if (!rows || !med || !nmed) return fail(SPX_E_ARG, "null pointer");
    // no pixel has more than 128 values: larger counts mean the same and cannot overflow m - nlow - nhigh
    if (nlow > spx::kDrzMaxFrames) nlow = spx::kDrzMaxFrames;
    if (nhigh > spx::kDrzMaxFrames) nhigh = spx::kDrzMaxFrames;
    const int lds = (int)spx::drizzle_median_lds_bytes(nactive);
    auto kern = spx::drizzle_median_kernel<T>;
    if (lds > 64 * 1024) {
        int dev = 0;
        SPX_HIP(hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(g_crr_mu);
        const auto key = std::make_pair(dev, reinterpret_cast<const void*>(kern));
        if (!g_crr_lds_ok.count(key)) {
            SPX_HIP(hipFuncSetAttribute(key.second, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)spx::drizzle_median_lds_bytes(spx::kDrzMaxFrames)));
            g_crr_lds_ok.insert(key);
        }
    }
    const int64_t tiles = (int64_t)((out_nx + spx::kDrzTileW - 1) / spx::kDrzTileW) *
                          ((out_ny + spx::kDrzTileH - 1) / spx::kDrzTileH);
    hipLaunchKernelGGL(kern, dim3(capped_grid(tiles, 1 << 20)), dim3(256), lds, reinterpret_cast<hipStream_t>(stream),
                       static_cast<const spx::DrizzleRow*>(rows), nframes, nactive, kernel, nlow, nhigh, out_ny, out_nx,
                       med, nmed);
    SPX_HIP(hipGetLastError());
    return 0;
}

bool cr_level_ok(double v) { return v - v == 0.0 && v >= 0.0; }

template <typename T>
int drizzle_cr(const void* rows, int nframes, int frame, int fny, int fnx, const float* med, const uint8_t* nmed,
               int out_ny, int out_nx, double rms_scalar, const T* rms_map, double sky, double gain, double snr1,
               double snr2, double scale1, double scale2, uint8_t* crmask, T* clean, void* stream) {
    if (const int rc = drizzle_sizes(nframes, 0, out_ny, out_nx)) return rc;
    if (frame < 0 || frame >= nframes) return fail(SPX_E_ARG, "frame must be a row of the table, 0..nframes-1");
    if (!cr_level_ok(snr1) || !cr_level_ok(snr2) || !cr_level_ok(scale1) || !cr_level_ok(scale2))
        return fail(SPX_E_ARG, "snr and scale must be finite and not negative");
    if (snr2 > snr1 || scale2 > scale1)
        return fail(SPX_E_ARG, "the second test must not be the stricter one: snr2 <= snr1 and scale2 <= scale1");
    if (!(sky - sky == 0.0)) return fail(SPX_E_ARG, "sky must be finite");
    if (!rows || !med || !nmed || !crmask || !clean) return fail(SPX_E_ARG, "null pointer");
    if (fny < 1 || fnx < 1 || (int64_t)fny * fnx >= 2147483647LL)
        return fail(SPX_E_SHAPE, "the frame must hold 1 .. 2^31 - 2 pixels");
    if (out_ny < spx::kCrMinOut || out_nx < spx::kCrMinOut)
        return fail(SPX_E_SHAPE, "the blot's quintic needs a median of 6 x 6 pixels at least");
    const spx::CrParams c = spx::host::cr_params(rms_scalar, sky, gain, snr1, snr2, scale1, scale2);
    const int64_t tiles = (int64_t)((fnx + spx::kDrzTileW - 1) / spx::kDrzTileW) *
                          ((fny + spx::kDrzTileH - 1) / spx::kDrzTileH);
    hipLaunchKernelGGL(spx::drizzle_cr_kernel<T>, dim3(capped_grid(tiles, 1 << 20)), dim3(256), spx::kCrLdsBytes,
                       reinterpret_cast<hipStream_t>(stream), static_cast<const spx::DrizzleRow*>(rows), frame, med,
                       nmed, out_ny, out_nx, rms_map, c, crmask, clean);
    SPX_HIP(hipGetLastError());
    return 0;
}

// minmed and the mask growth (spx_minmed_kernels.h)
template <typename T>
int drizzle_minmed(const void* rows, int nframes, int nactive, int kernel, int nlow, int nhigh, const double* table,
                   double nsigma1, double nsigma2, int grow, int out_ny, int out_nx, float* md, float* lo,
                   uint8_t* bits, float* med, uint8_t* nmed, uint8_t* minmed, void* stream) {
    if (const int rc = drizzle_sizes(nframes, kernel, out_ny, out_nx)) return rc;
    if (nactive < 1 || nactive > nframes) return fail(SPX_E_ARG, "nactive must be 1..nframes");
    if (nlow < 0 || nhigh < 0) return fail(SPX_E_ARG, "nlow and nhigh must not be negative");
    if (!cr_level_ok(nsigma1) || !cr_level_ok(nsigma2))
        return fail(SPX_E_ARG, "nsigma must be finite and not negative");
    if (nsigma2 > nsigma1) return fail(SPX_E_ARG, "the second test must not be the stricter one: nsigma2 <= nsigma1");
    if (grow < 0 || grow > spx::kMmMaxGrow) return fail(SPX_E_ARG, "grow must be 0..8");
    if (!rows || !table || !md || !lo || !bits || !med || !nmed || !minmed) return fail(SPX_E_ARG, "null pointer");
    if (med == md || med == lo || minmed == bits || minmed == nmed || bits == nmed)
        return fail(SPX_E_ARG, "the planes of the two passes must be distinct: no pass reads a plane it writes");
    if (nlow > spx::kDrzMaxFrames) nlow = spx::kDrzMaxFrames;
    if (nhigh > spx::kDrzMaxFrames) nhigh = spx::kDrzMaxFrames;
    const int lds = (int)spx::drizzle_median_lds_bytes(nactive);
    auto kern = spx::drizzle_minmed_kernel<T>;
    if (lds > 64 * 1024) {
        int dev = 0;
        SPX_HIP(hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(g_crr_mu);
        const auto key = std::make_pair(dev, reinterpret_cast<const void*>(kern));
        if (!g_crr_lds_ok.count(key)) {
            SPX_HIP(hipFuncSetAttribute(key.second, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)spx::drizzle_median_lds_bytes(spx::kDrzMaxFrames)));
            g_crr_lds_ok.insert(key);
        }
    }
    const int64_t tiles = (int64_t)((out_nx + spx::kDrzTileW - 1) / spx::kDrzTileW) *
                          ((out_ny + spx::kDrzTileH - 1) / spx::kDrzTileH);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(kern, dim3(capped_grid(tiles, 1 << 20)), dim3(256), lds, s,
                       static_cast<const spx::DrizzleRow*>(rows), nframes, nactive, kernel, nlow, nhigh, table, nsigma1,
                       nsigma2, out_ny, out_nx, md, lo, bits, nmed);
    SPX_HIP(hipGetLastError());
    hipLaunchKernelGGL(spx::minmed_grow_kernel, dim3(capped_grid(tiles, 1 << 20)), dim3(256), spx::kMmGrowLdsBytes, s,
                       md, lo, bits, grow, out_ny, out_nx, med, minmed);
    SPX_HIP(hipGetLastError());
    return 0;
}

template <typename T>
int drizzle_cr_grow(const void* rows, int nframes, int frame, int fny, int fnx, const float* med, const uint8_t* nmed,
                    int out_ny, int out_nx, double rms_scalar, const T* rms_map, const uint8_t* seed, int grow,
                    int ctegrow, int ctedir, uint8_t* crmask, T* clean, void* stream) {
    if (const int rc = drizzle_sizes(nframes, 0, out_ny, out_nx)) return rc;
    if (frame < 0 || frame >= nframes) return fail(SPX_E_ARG, "frame must be a row of the table, 0..nframes-1");
    if (grow < 1 || grow > 2 * spx::kCrGrowMaxHalf + 1 || !(grow & 1)) return fail(SPX_E_ARG, "grow must be odd, 1..9");
    if (ctegrow < 0 || ctegrow > spx::kCrGrowMaxCte) return fail(SPX_E_ARG, "ctegrow must be 0..64");
    if (ctedir < -1 || ctedir > 1) return fail(SPX_E_ARG, "ctedir must be -1, 0 or +1");
    if (!rows || !med || !nmed || !seed || !crmask || !clean) return fail(SPX_E_ARG, "null pointer");
    if (seed == crmask) return fail(SPX_E_ARG, "the seed mask and the grown mask must be distinct planes");
    if (fny < 1 || fnx < 1 || (int64_t)fny * fnx >= 2147483647LL)
        return fail(SPX_E_SHAPE, "the frame must hold 1 .. 2^31 - 2 pixels");
    if (out_ny < spx::kCrMinOut || out_nx < spx::kCrMinOut)
        return fail(SPX_E_SHAPE, "the blot's quintic needs a median of 6 x 6 pixels at least");
    const int64_t tiles = (int64_t)((fnx + spx::kDrzTileW - 1) / spx::kDrzTileW) *
                          ((fny + spx::kDrzTileH - 1) / spx::kDrzTileH);
    hipLaunchKernelGGL(spx::drizzle_cr_grow_kernel<T>, dim3(capped_grid(tiles, 1 << 20)), dim3(256),
                       spx::kCrGrowLdsBytes, reinterpret_cast<hipStream_t>(stream),
                       static_cast<const spx::DrizzleRow*>(rows), frame, med, nmed, out_ny, out_nx, rms_scalar, rms_map,
                       seed, grow, ctegrow, ctedir, crmask, clean);
    SPX_HIP(hipGetLastError());
    return 0;
}
}  // namespace

extern "C" {

int spx_drizzle_rows(const void* const* frames, const void* const* weights, const uint8_t* const* masks,
                     const int32_t* shapes, const double* maps_f64, const uint8_t* active, int nframes,
                     double pixfrac, int kernel, int out_ny, int out_nx, void* out_rows) {
    if (const int rc = drizzle_sizes(nframes, kernel, out_ny, out_nx)) return rc;
    if (!(pixfrac > 0.0 && pixfrac <= 1.0)) return fail(SPX_E_ARG, "pixfrac must lie in (0, 1]");
    if (!frames || !shapes || !maps_f64 || !out_rows) return fail(SPX_E_ARG, "null pointer");
    for (int k = 0; k < nframes; ++k) {
        if (!frames[k]) return fail(SPX_E_ARG, "null pointer: frame " + std::to_string(k));
        const int ny = shapes[2 * k], nx = shapes[2 * k + 1];
        if (ny < 1 || nx < 1 || (int64_t)ny * nx >= 2147483647LL)
            return fail(SPX_E_SHAPE, "frame " + std::to_string(k) + " must hold 1 .. 2^31 - 2 pixels");
    }
    std::vector<spx::DrizzleRow> rows((size_t)nframes);
    for (int k = 0; k < nframes; ++k) {
        const int rc = spx::host::drizzle_pack_row(frames[k], weights ? weights[k] : nullptr,
                                                   masks ? masks[k] : nullptr, shapes[2 * k], shapes[2 * k + 1],
                                                   active ? active[k] : 1, maps_f64 + 6 * k, pixfrac, kernel,
                                                   &rows[(size_t)k]);
        if (rc == 1) return fail(SPX_E_ARG, "the map of frame " + std::to_string(k) + " has an entry that is not finite");
        if (rc == 2) return fail(SPX_E_ARG, "the map of frame " + std::to_string(k) + " is singular");
        if (rc == 3)
            return fail(SPX_E_SHAPE, "the map of frame " + std::to_string(k) +
                                         " shrinks the frame so far that one output pixel gathers from more than 8 x 8");
    }
    memcpy(out_rows, rows.data(), rows.size() * sizeof(spx::DrizzleRow));      // nothing is written on an error
    return 0;
}
int spx_drizzle_f32(const void* rows, int nframes, int kernel, double fill, int out_ny, int out_nx, float* out_sci,
                    float* out_wht, int32_t* out_ctx, void* stream) {
    return drizzle<float>(rows, nframes, kernel, fill, out_ny, out_nx, out_sci, out_wht, out_ctx, stream);
}
int spx_drizzle_f64(const void* rows, int nframes, int kernel, double fill, int out_ny, int out_nx, double* out_sci,
                    float* out_wht, int32_t* out_ctx, void* stream) {
    return drizzle<double>(rows, nframes, kernel, fill, out_ny, out_nx, out_sci, out_wht, out_ctx, stream);
}
int spx_drizzle_poly_rows(const void* const* frames, const void* const* weights, const uint8_t* const* masks,
                          const int32_t* shapes, const double* coef_f64, const int32_t* degree,
                          const double* center_f64, const uint8_t* active, int nframes, double pixfrac, int kernel,
                          int out_ny, int out_nx, void* out_rows) {
    if (const int rc = drizzle_sizes(nframes, kernel, out_ny, out_nx)) return rc;
    if (!(pixfrac > 0.0 && pixfrac <= 1.0)) return fail(SPX_E_ARG, "pixfrac must lie in (0, 1]");
    if (!frames || !shapes || !coef_f64 || !degree || !center_f64 || !out_rows) return fail(SPX_E_ARG, "null pointer");
    for (int k = 0; k < nframes; ++k) {
        if (!frames[k]) return fail(SPX_E_ARG, "null pointer: frame " + std::to_string(k));
        const int ny = shapes[2 * k], nx = shapes[2 * k + 1];
        if (ny < 1 || nx < 1 || (int64_t)ny * nx >= 2147483647LL)
            return fail(SPX_E_SHAPE, "frame " + std::to_string(k) + " must hold 1 .. 2^31 - 2 pixels");
    }
    std::vector<spx::DrizzlePolyRow> rows((size_t)nframes);
    for (int k = 0; k < nframes; ++k) {
        const int rc = spx::host::drizzle_poly_pack_row(
            frames[k], weights ? weights[k] : nullptr, masks ? masks[k] : nullptr, shapes[2 * k], shapes[2 * k + 1],
            active ? active[k] : 1, coef_f64 + (size_t)k * 2 * spx::kDrzPolyTerms, degree[k], center_f64 + 2 * k,
            pixfrac, kernel, &rows[(size_t)k]);
        const std::string which = "the map of frame " + std::to_string(k);
        if (rc == 1) return fail(SPX_E_ARG, which + " has a coefficient or a centre that is not finite");
        if (rc == 2)
            return fail(SPX_E_ARG, which + " is singular: its Jacobian determinant is zero, not finite or changes "
                                           "sign inside the frame");
        if (rc == 3)
            return fail(SPX_E_SHAPE, which + " shrinks or bends the frame so far that one output pixel gathers from "
                                             "more than 8 x 8");
        if (rc == 4) return fail(SPX_E_ARG, which + " has a degree outside 1 .. 5");
    }
    memcpy(out_rows, rows.data(), rows.size() * sizeof(spx::DrizzlePolyRow));  // nothing is written on an error
    return 0;
}
int spx_drizzle_poly_f32(const void* rows, int nframes, int kernel, double fill, int out_ny, int out_nx, float* out_sci,
                         float* out_wht, int32_t* out_ctx, void* stream) {
    return drizzle_poly<float>(rows, nframes, kernel, fill, out_ny, out_nx, out_sci, out_wht, out_ctx, stream);
}
int spx_drizzle_poly_f64(const void* rows, int nframes, int kernel, double fill, int out_ny, int out_nx,
                         double* out_sci, float* out_wht, int32_t* out_ctx, void* stream) {
    return drizzle_poly<double>(rows, nframes, kernel, fill, out_ny, out_nx, out_sci, out_wht, out_ctx, stream);
}
int spx_drizzle_median_f32(const void* rows, int nframes, int nactive, int kernel, int nlow, int nhigh, int out_ny,
                           int out_nx, float* out_med, uint8_t* out_nmed, void* stream) {
    return drizzle_median<float>(rows, nframes, nactive, kernel, nlow, nhigh, out_ny, out_nx, out_med, out_nmed, stream);
}
int spx_drizzle_median_f64(const void* rows, int nframes, int nactive, int kernel, int nlow, int nhigh, int out_ny,
                           int out_nx, float* out_med, uint8_t* out_nmed, void* stream) {
    return drizzle_median<double>(rows, nframes, nactive, kernel, nlow, nhigh, out_ny, out_nx, out_med, out_nmed, stream);
}
int spx_drizzle_cr_f32(const void* rows, int nframes, int frame, int fny, int fnx, const float* med,
                       const uint8_t* nmed, int out_ny, int out_nx, double rms_scalar, const float* rms_map, double sky,
                       double gain, double snr1, double snr2, double scale1, double scale2, uint8_t* out_crmask,
                       float* out_clean, void* stream) {
    return drizzle_cr<float>(rows, nframes, frame, fny, fnx, med, nmed, out_ny, out_nx, rms_scalar, rms_map, sky, gain,
                             snr1, snr2, scale1, scale2, out_crmask, out_clean, stream);
}
int spx_drizzle_cr_f64(const void* rows, int nframes, int frame, int fny, int fnx, const float* med,
                       const uint8_t* nmed, int out_ny, int out_nx, double rms_scalar, const double* rms_map,
                       double sky, double gain, double snr1, double snr2, double scale1, double scale2,
                       uint8_t* out_crmask, double* out_clean, void* stream) {
    return drizzle_cr<double>(rows, nframes, frame, fny, fnx, med, nmed, out_ny, out_nx, rms_scalar, rms_map, sky, gain,
                              snr1, snr2, scale1, scale2, out_crmask, out_clean, stream);
}
int spx_drizzle_minmed_f32(const void* rows, int nframes, int nactive, int kernel, int nlow, int nhigh,
                           const double* table_f64, double nsigma1, double nsigma2, int grow, int out_ny, int out_nx,
                           float* out_md, float* out_lo, uint8_t* out_bits, float* out_med, uint8_t* out_nmed,
                           uint8_t* out_minmed, void* stream) {
    return drizzle_minmed<float>(rows, nframes, nactive, kernel, nlow, nhigh, table_f64, nsigma1, nsigma2, grow, out_ny,
                                 out_nx, out_md, out_lo, out_bits, out_med, out_nmed, out_minmed, stream);
}
int spx_drizzle_minmed_f64(const void* rows, int nframes, int nactive, int kernel, int nlow, int nhigh,
                           const double* table_f64, double nsigma1, double nsigma2, int grow, int out_ny, int out_nx,
                           float* out_md, float* out_lo, uint8_t* out_bits, float* out_med, uint8_t* out_nmed,
                           uint8_t* out_minmed, void* stream) {
    return drizzle_minmed<double>(rows, nframes, nactive, kernel, nlow, nhigh, table_f64, nsigma1, nsigma2, grow, out_ny,
                                  out_nx, out_md, out_lo, out_bits, out_med, out_nmed, out_minmed, stream);
}
int spx_drizzle_cr_grow_f32(const void* rows, int nframes, int frame, int fny, int fnx, const float* med,
                            const uint8_t* nmed, int out_ny, int out_nx, double rms_scalar, const float* rms_map,
                            const uint8_t* seed, int grow, int ctegrow, int ctedir, uint8_t* out_crmask,
                            float* clean, void* stream) {
    return drizzle_cr_grow<float>(rows, nframes, frame, fny, fnx, med, nmed, out_ny, out_nx, rms_scalar, rms_map, seed,
                                  grow, ctegrow, ctedir, out_crmask, clean, stream);
}
int spx_drizzle_cr_grow_f64(const void* rows, int nframes, int frame, int fny, int fnx, const float* med,
                            const uint8_t* nmed, int out_ny, int out_nx, double rms_scalar, const double* rms_map,
                            const uint8_t* seed, int grow, int ctegrow, int ctedir, uint8_t* out_crmask,
                            double* clean, void* stream) {
    return drizzle_cr_grow<double>(rows, nframes, frame, fny, fnx, med, nmed, out_ny, out_nx, rms_scalar, rms_map, seed,
                                   grow, ctegrow, ctedir, out_crmask, clean, stream);
}
int spx_measure_errors_f32(const float* frame, const uint8_t* bad_mask, double bkg_scalar, const float* bkg_map,
                           double rms_scalar, const float* rms_map, double gain, const int32_t* labels, int fny,
                           int fnx, int nlabels, const int32_t* boxes, const double* table_f64,
                           double* out_errors_f64, int32_t* out_eflags_i32, void* stream) {
    return measure_errors<float>(frame, bad_mask, bkg_scalar, bkg_map, rms_scalar, rms_map, gain, labels, fny, fnx,
                                 nlabels, boxes, table_f64, out_errors_f64, out_eflags_i32, stream);
}
int spx_measure_errors_f64(const double* frame, const uint8_t* bad_mask, double bkg_scalar, const double* bkg_map,
                           double rms_scalar, const double* rms_map, double gain, const int32_t* labels, int fny,
                           int fnx, int nlabels, const int32_t* boxes, const double* table_f64,
                           double* out_errors_f64, int32_t* out_eflags_i32, void* stream) {
    return measure_errors<double>(frame, bad_mask, bkg_scalar, bkg_map, rms_scalar, rms_map, gain, labels, fny, fnx,
                                  nlabels, boxes, table_f64, out_errors_f64, out_eflags_i32, stream);
}
size_t spx_detect_workspace_bytes(int fny, int fnx) {
    if (fny < 1 || fnx < 1 || (int64_t)fny * fnx >= 2147483647LL) return 0;
    return detect_layout((int64_t)fny * fnx).total;
}
int spx_detect_label_f32(const float* frame, const uint8_t* bad_mask, float thr_scalar, const float* thr_map,
                         const float* filter, int fky, int fkx, int fny, int fnx, int connectivity,
                         int min_area, void* work, size_t work_bytes, int32_t* out_labels,
                         int32_t* out_nlabels, void* stream) {
    return detect_label<float>(frame, bad_mask, thr_scalar, thr_map, filter, fky, fkx, fny, fnx, connectivity,
                               min_area, work, work_bytes, out_labels, out_nlabels, stream);
}
int spx_detect_label_f64(const double* frame, const uint8_t* bad_mask, double thr_scalar, const float* thr_map,
                         const double* filter, int fky, int fkx, int fny, int fnx, int connectivity,
                         int min_area, void* work, size_t work_bytes, int32_t* out_labels,
                         int32_t* out_nlabels, void* stream) {
    return detect_label<double>(frame, bad_mask, thr_scalar, thr_map, filter, fky, fkx, fny, fnx, connectivity,
                                min_area, work, work_bytes, out_labels, out_nlabels, stream);
}
int spx_measure_labels_f32(const float* frame, const uint8_t* bad_mask, double bkg_scalar, const float* bkg_map,
                           const int32_t* labels, int fny, int fnx, int nlabels, const int32_t* boxes,
                           double* out_table_f64, int32_t* out_flags_i32, void* stream) {
    return measure_labels<float>(frame, bad_mask, bkg_scalar, bkg_map, labels, fny, fnx, nlabels, boxes,
                                 out_table_f64, out_flags_i32, stream);
}
int spx_measure_labels_f64(const double* frame, const uint8_t* bad_mask, double bkg_scalar, const double* bkg_map,
                           const int32_t* labels, int fny, int fnx, int nlabels, const int32_t* boxes,
                           double* out_table_f64, int32_t* out_flags_i32, void* stream) {
    return measure_labels<double>(frame, bad_mask, bkg_scalar, bkg_map, labels, fny, fnx, nlabels, boxes,
                                  out_table_f64, out_flags_i32, stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------
// deblending (spx_deblend_kernels.h).  Workspace: the detection's layout (R | cnt | chunk sums | status) for the
// numbering kernels, then per-parent flags int32 [nlabels + 1], then min(nlabels, kDebSlots) slots of 36 B per
// pixel of the largest box a parent can have (min(65536, fny * fnx)) for the parents that do not fit LDS.
// ---------------------------------------------------------------------------------------------------------
namespace {
struct DeblendLayout {
    DetectLayout det;
    size_t pflag, slots, slot_bytes, total;
    int nslots;
};
DeblendLayout deblend_layout(int64_t npix, int nlabels) {
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    DeblendLayout d;
    d.det = detect_layout(npix);
    d.pflag = d.det.total;
    d.slots = d.pflag + up(((size_t)nlabels + 1) * 4);
    const int64_t most = npix < spx::kDebMaxBoxPixels ? npix : spx::kDebMaxBoxPixels;
    d.slot_bytes = most > spx::kDebLdsPixels ? up((size_t)most * spx::kDebBytesPerPixel) : 0;
    d.nslots = nlabels < spx::kDebSlots ? nlabels : spx::kDebSlots;
    d.total = d.slots + d.slot_bytes * (size_t)d.nslots;
    return d;
}

template <typename T>
int deblend_labels(const T* frame, const uint8_t* bad, const T* filter, int fky, int fkx, int fny, int fnx,
                   const int32_t* labels, int nlabels, const int32_t* boxes, int conn, int min_area, int nlevels,
                   double contrast, int mode, void* work, size_t work_bytes, int32_t* out_labels,
                   int32_t* out_parent, int32_t* out_dflags, int max_out, int32_t* out_nlabels, void* stream) {
    if (!frame || !labels || !boxes || !out_labels || !out_parent || !out_dflags || !out_nlabels)
        return fail(SPX_E_ARG, "null pointer");
    if (fny < 1 || fnx < 1 || (int64_t)fny * fnx >= 2147483647LL)
        return fail(SPX_E_SHAPE, "the frame must hold 1 .. 2^31 - 2 pixels");
    if (nlabels < 0 || max_out < 0) return fail(SPX_E_ARG, "negative label count or max_out");
    if (conn != 4 && conn != 8) return fail(SPX_E_ARG, "connectivity must be 4 or 8");
    if (min_area < 1) return fail(SPX_E_ARG, "min_area must be at least 1");
    if (nlevels < 1 || nlevels > 63 || ((nlevels + 1) & nlevels))
        return fail(SPX_E_ARG, "nlevels + 1 must be a power of two in 2..64");
    if (!(contrast >= 0.0 && contrast <= 1.0)) return fail(SPX_E_ARG, "contrast must lie in 0..1");
    if (mode != 0 && mode != 1) return fail(SPX_E_ARG, "mode must be 0 (exponential) or 1 (linear)");
    if (!filter) fky = fkx = 1;
    if (fky < 1 || fkx < 1 || !(fky & 1) || !(fkx & 1) || fky > spx::kDetMaxFilter || fkx > spx::kDetMaxFilter)
        return fail(SPX_E_ARG, "filter sides must be odd and at most 7");
    const int npix = fny * fnx;
    const DeblendLayout lay = deblend_layout(npix, nlabels);
    if (!work || work_bytes < lay.total)
        return fail(SPX_E_WORKSPACE, "workspace missing or smaller than spx_deblend_workspace_bytes(fny, fnx, nlabels)");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* w = static_cast<char*>(work);
    int32_t* R = reinterpret_cast<int32_t*>(w + lay.det.r);
    int32_t* cnt = reinterpret_cast<int32_t*>(w + lay.det.cnt);
    int32_t* sums = reinterpret_cast<int32_t*>(w + lay.det.sums);
    int32_t* status = reinterpret_cast<int32_t*>(w + lay.det.status);
    int32_t* pflag = reinterpret_cast<int32_t*>(w + lay.pflag);
    unsigned char* slots = reinterpret_cast<unsigned char*>(w + lay.slots);
    SPX_HIP(hipMemsetAsync(status, 0, 4, s));
    SPX_HIP(hipMemsetAsync(R, 0, (size_t)npix * 4, s));
    SPX_HIP(hipMemsetAsync(pflag, 0, ((size_t)nlabels + 1) * 4, s));
    if (nlabels > 0) {
        // one launch per storage class, each over all labels (a workgroup skips the other classes' parents)
        hipLaunchKernelGGL((spx::deblend_parents_kernel<T, 64, false>), dim3(capped_grid(nlabels, 1 << 20)), dim3(64),
                           spx::deb_lds_bytes(spx::kDebWavePixels), s, frame, bad, filter, fky, fkx, fny, fnx, labels,
                           nlabels, boxes, conn, min_area, nlevels, contrast, mode, 0, spx::kDebWavePixels, slots,
                           lay.slot_bytes, R, cnt, pflag, status);
        SPX_HIP(hipGetLastError());
        const int mid[3] = {spx::kDebWavePixels, spx::kDebMidPixels, spx::kDebLdsPixels};
        for (int c = 0; c < 2 && npix > mid[c]; ++c) {
            hipLaunchKernelGGL((spx::deblend_parents_kernel<T, 256, false>), dim3(capped_grid(nlabels, 1 << 20)),
                               dim3(256), spx::deb_lds_bytes(mid[c + 1]), s, frame, bad, filter, fky, fkx, fny, fnx,
                               labels, nlabels, boxes, conn, min_area, nlevels, contrast, mode, mid[c] + 1, mid[c + 1],
                               slots, lay.slot_bytes, R, cnt, pflag, status);
            SPX_HIP(hipGetLastError());
        }
        if (npix > spx::kDebLdsPixels) {
            hipLaunchKernelGGL((spx::deblend_parents_kernel<T, spx::kDebWsThreads, true>), dim3((unsigned)lay.nslots),
                               dim3(spx::kDebWsThreads), spx::deb_lds_bytes(0), s, frame, bad, filter, fky, fkx, fny, fnx,
                               labels, nlabels, boxes, conn, min_area, nlevels, contrast, mode, spx::kDebLdsPixels + 1,
                               spx::kDebMaxBoxPixels, slots, lay.slot_bytes, R, cnt, pflag, status);
            SPX_HIP(hipGetLastError());
        }
    }
    // number the final segments as detect_label numbers components: every segment has cnt[first pixel] = 1
    const int64_t nchunks = ((int64_t)npix + spx::kDetChunk - 1) / spx::kDetChunk;
    hipLaunchKernelGGL(spx::detect_flag_count_kernel, dim3(capped_grid(nchunks)), dim3(256), spx::kDetScanLdsBytes,
                       s, R, cnt, npix, 1, sums);
    SPX_HIP(hipGetLastError());
    hipLaunchKernelGGL(spx::detect_scan_blocks_kernel, dim3(1), dim3(256), spx::kDetScanLdsBytes, s, sums, nchunks,
                       status, out_nlabels);
    SPX_HIP(hipGetLastError());
    hipLaunchKernelGGL(spx::detect_assign_kernel, dim3(capped_grid(nchunks)), dim3(256), spx::kDetScanLdsBytes, s,
                       R, cnt, npix, 1, sums);
    SPX_HIP(hipGetLastError());
    hipLaunchKernelGGL(spx::detect_relabel_kernel, dim3(capped_grid(((int64_t)npix + 255) / 256)), dim3(256), 0, s,
                       R, cnt, npix, out_labels);
    SPX_HIP(hipGetLastError());
    hipLaunchKernelGGL(spx::deblend_table_kernel, dim3(capped_grid(((int64_t)npix + 255) / 256)), dim3(256), 0, s, R,
                       cnt, labels, pflag, npix, nlabels, max_out, out_parent, out_dflags);
    SPX_HIP(hipGetLastError());
    return 0;
}
}  // namespace

extern "C" {

size_t spx_deblend_workspace_bytes(int fny, int fnx, int nlabels) {
    if (fny < 1 || fnx < 1 || (int64_t)fny * fnx >= 2147483647LL || nlabels < 0) return 0;
    return deblend_layout((int64_t)fny * fnx, nlabels).total;
}
int spx_deblend_labels_f32(const float* frame, const uint8_t* bad_mask, const float* filter, int fky, int fkx,
                           int fny, int fnx, const int32_t* labels, int nlabels, const int32_t* boxes,
                           int connectivity, int min_area, int nlevels, double contrast, int mode, void* work,
                           size_t work_bytes, int32_t* out_labels, int32_t* out_parent, int32_t* out_dflags,
                           int max_out, int32_t* out_nlabels, void* stream) {
    return deblend_labels<float>(frame, bad_mask, filter, fky, fkx, fny, fnx, labels, nlabels, boxes, connectivity,
                                 min_area, nlevels, contrast, mode, work, work_bytes, out_labels, out_parent,
                                 out_dflags, max_out, out_nlabels, stream);
}
int spx_deblend_labels_f64(const double* frame, const uint8_t* bad_mask, const double* filter, int fky, int fkx,
                           int fny, int fnx, const int32_t* labels, int nlabels, const int32_t* boxes,
                           int connectivity, int min_area, int nlevels, double contrast, int mode, void* work,
                           size_t work_bytes, int32_t* out_labels, int32_t* out_parent, int32_t* out_dflags,
                           int max_out, int32_t* out_nlabels, void* stream) {
    return deblend_labels<double>(frame, bad_mask, filter, fky, fkx, fny, fnx, labels, nlabels, boxes, connectivity,
                                  min_area, nlevels, contrast, mode, work, work_bytes, out_labels, out_parent,
                                  out_dflags, max_out, out_nlabels, stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------
// background and noise maps (spx_background_kernels.h).  Workspace: float64 planes [2 meshes][6][ncy * ncx]
// (plane 0 of mesh 0 / 1 = the FILTERED background / rms mesh, which callers may read back), then a 256-byte
// control block on a 256-byte boundary.
// ---------------------------------------------------------------------------------------------------------
namespace {
struct BackgroundLayout {
    size_t ctl, total;
};
BackgroundLayout background_layout(int64_t ncells) {
    BackgroundLayout b;
    b.ctl = ((size_t)ncells * 8 * 2 * spx::kBkgPlanes + 255) / 256 * 256;
    b.total = b.ctl + 256;
    return b;
}
int background_shape(int fny, int fnx, int bh, int bw, size_t elem) {
    if (fny < 1 || fnx < 1 || (int64_t)fny * fnx >= 2147483647LL)
        return fail(SPX_E_SHAPE, "the frame must hold 1 .. 2^31 - 2 pixels");
    if (bh < spx::kBkgMinBox || bw < spx::kBkgMinBox || bh > spx::kBkgMaxBox || bw > spx::kBkgMaxBox ||
        bh * bw > spx::bkg_max_cell_pixels(elem))
        return fail(SPX_E_SHAPE, "mesh cells must be 8..128 pixels a side and hold at most 16384 (float64: 8192) pixels");
    return 0;
}
std::mutex g_bkg_mu;
std::set<std::pair<int, const void*>> g_bkg_lds_ok;       // (device, kernel) whose dynamic-LDS limit is raised

template <typename T>
int background_mesh(const T* frame, const uint8_t* bad, const int32_t* labels, int fny, int fnx, int bh, int bw,
                    double kappa, int max_iters, double min_good_fraction, double* mesh_bkg, double* mesh_rms,
                    int32_t* mesh_ngood, void* stream) {
    if (!frame || !mesh_bkg || !mesh_rms || !mesh_ngood) return fail(SPX_E_ARG, "null pointer");
    if (!(kappa > 0.0) || !(kappa - kappa == 0.0)) return fail(SPX_E_ARG, "kappa must be positive and finite");
    if (max_iters < 0) return fail(SPX_E_ARG, "max_iters must not be negative");
    if (!(min_good_fraction >= 0.0 && min_good_fraction <= 1.0))
        return fail(SPX_E_ARG, "min_good_fraction must lie in 0..1");
    const int rc = background_shape(fny, fnx, bh, bw, sizeof(T));
    if (rc) return rc;
    const int lds = (int)spx::bkg_cell_lds_bytes(sizeof(T), bh, bw);
    auto kern = spx::bkg_cell_kernel<T>;
    if (lds > 48 * 1024) {
        int dev = 0;
        SPX_HIP(hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(g_bkg_mu);
        const auto key = std::make_pair(dev, reinterpret_cast<const void*>(kern));
        if (!g_bkg_lds_ok.count(key)) {
            SPX_HIP(hipFuncSetAttribute(key.second, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(spx::kBkgRedSlots * 8 + 64 * 1024)));
            g_bkg_lds_ok.insert(key);
        }
    }
    const int64_t ncells = (int64_t)((fny + bh - 1) / bh) * ((fnx + bw - 1) / bw);
    hipLaunchKernelGGL(kern, dim3(capped_grid(ncells, 1 << 20)), dim3(256), lds, reinterpret_cast<hipStream_t>(stream),
                       frame, bad, labels, fny, fnx, bh, bw, kappa, max_iters, min_good_fraction, mesh_bkg, mesh_rms,
                       mesh_ngood, (double*)nullptr);
    SPX_HIP(hipGetLastError());
    return 0;
}

template <typename T>
int background_maps(const double* mesh_bkg, const double* mesh_rms, const int32_t* mesh_ngood, int ncy, int ncx,
                    int bh, int bw, int filter_size, int fny, int fnx, double nsigma, void* work, size_t work_bytes,
                    T* bkg_out, T* rms_out, float* thr_out, int32_t* status, void* stream) {
    if (!mesh_bkg || !mesh_rms || !mesh_ngood || !status) return fail(SPX_E_ARG, "null pointer");
    if (!bkg_out && !rms_out && !thr_out) return fail(SPX_E_ARG, "no output map");
    if (filter_size != 1 && filter_size != 3 && filter_size != 5 && filter_size != 7)
        return fail(SPX_E_ARG, "filter_size must be 1, 3, 5 or 7");
    const int rc = background_shape(fny, fnx, bh, bw, sizeof(T));
    if (rc) return rc;
    if (ncy != (fny + bh - 1) / bh || ncx != (fnx + bw - 1) / bw)
        return fail(SPX_E_SHAPE, "mesh size must be ceil(fny / bh) x ceil(fnx / bw)");
    const int64_t nc = (int64_t)ncy * ncx;
    const BackgroundLayout lay = background_layout(nc);
    if (!work || work_bytes < lay.total)
        return fail(SPX_E_WORKSPACE, "workspace missing or smaller than spx_background_workspace_bytes(fny, fnx, bh, bw)");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    double* planes = static_cast<double*>(work);
    int32_t* ctl = reinterpret_cast<int32_t*>(static_cast<char*>(work) + lay.ctl);
    double* fb = planes;
    double* fr = planes + (int64_t)spx::kBkgPlanes * nc;
    SPX_HIP(hipMemsetAsync(ctl, 0, 256, s));
    SPX_HIP(hipMemsetAsync(status, 0, 4, s));
    hipLaunchKernelGGL(spx::bkg_filter_kernel, dim3(capped_grid((nc + 255) / 256)), dim3(256), 0, s, mesh_bkg, mesh_rms,
                       mesh_ngood, ncy, ncx, filter_size, fb, fr, ctl);
    SPX_HIP(hipGetLastError());
    hipLaunchKernelGGL(spx::bkg_global_kernel, dim3(1), dim3(256), spx::kBkgGlobalLdsBytes, s, mesh_bkg, mesh_rms,
                       mesh_ngood, nc, fb, fr, ctl, status);
    SPX_HIP(hipGetLastError());
    for (int phase = 0; phase < 2; ++phase) {
        const int64_t lines = 2 * (int64_t)(phase == 0 ? ncx + ncy : ncx);
        hipLaunchKernelGGL(spx::bkg_spline_kernel, dim3(capped_grid((lines + 255) / 256)), dim3(256), 0, s, planes, ncy,
                           ncx, phase);
        SPX_HIP(hipGetLastError());
    }
    const int64_t groups = (int64_t)fny * ((fnx + 3) / 4);
    hipLaunchKernelGGL(spx::bkg_expand_kernel<T>, dim3(capped_grid((groups + 255) / 256, 1 << 20)), dim3(256), 0, s,
                       planes, ncy, ncx, bh, bw, fny, fnx, nsigma, bkg_out, rms_out, thr_out);
    SPX_HIP(hipGetLastError());
    return 0;
}
}  // namespace

extern "C" {

size_t spx_background_workspace_bytes(int fny, int fnx, int bh, int bw) {
    if (fny < 1 || fnx < 1 || (int64_t)fny * fnx >= 2147483647LL) return 0;
    if (bh < spx::kBkgMinBox || bw < spx::kBkgMinBox || bh > spx::kBkgMaxBox || bw > spx::kBkgMaxBox ||
        bh * bw > spx::bkg_max_cell_pixels(4))
        return 0;
    return background_layout((int64_t)((fny + bh - 1) / bh) * ((fnx + bw - 1) / bw)).total;
}
int spx_background_mesh_f32(const float* frame, const uint8_t* bad_mask, const int32_t* labels, int fny, int fnx,
                            int bh, int bw, double kappa, int max_iters, double min_good_fraction,
                            double* mesh_bkg, double* mesh_rms, int32_t* mesh_ngood, void* stream) {
    return background_mesh<float>(frame, bad_mask, labels, fny, fnx, bh, bw, kappa, max_iters, min_good_fraction,
                                  mesh_bkg, mesh_rms, mesh_ngood, stream);
}
int spx_background_mesh_f64(const double* frame, const uint8_t* bad_mask, const int32_t* labels, int fny, int fnx,
                            int bh, int bw, double kappa, int max_iters, double min_good_fraction,
                            double* mesh_bkg, double* mesh_rms, int32_t* mesh_ngood, void* stream) {
    return background_mesh<double>(frame, bad_mask, labels, fny, fnx, bh, bw, kappa, max_iters, min_good_fraction,
                                   mesh_bkg, mesh_rms, mesh_ngood, stream);
}
int spx_background_maps_f32(const double* mesh_bkg, const double* mesh_rms, const int32_t* mesh_ngood, int ncy,
                            int ncx, int bh, int bw, int filter_size, int fny, int fnx, double nsigma, void* work,
                            size_t work_bytes, float* bkg_out, float* rms_out, float* thr_out, int32_t* status,
                            void* stream) {
    return background_maps<float>(mesh_bkg, mesh_rms, mesh_ngood, ncy, ncx, bh, bw, filter_size, fny, fnx, nsigma,
                                  work, work_bytes, bkg_out, rms_out, thr_out, status, stream);
}
int spx_background_maps_f64(const double* mesh_bkg, const double* mesh_rms, const int32_t* mesh_ngood, int ncy,
                            int ncx, int bh, int bw, int filter_size, int fny, int fnx, double nsigma, void* work,
                            size_t work_bytes, double* bkg_out, double* rms_out, float* thr_out, int32_t* status,
                            void* stream) {
    return background_maps<double>(mesh_bkg, mesh_rms, mesh_ngood, ncy, ncx, bh, bw, filter_size, fny, fnx, nsigma,
                                   work, work_bytes, bkg_out, rms_out, thr_out, status, stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------
// sigma-clipped statistics of whole frames (spx_sky_kernels.h).  Workspace: [nframes] state records, the frames'
// histograms, the moment partials; cleared by the call.  The call only enqueues: a memset and kernels.
// ---------------------------------------------------------------------------------------------------------
namespace {
template <typename T>
int sky_stats(const void* const* frames, const void* const* weights, const uint8_t* const* masks,
              const int32_t* shapes, int nframes, double lower, double upper, double lsigma, double usigma,
              int max_iters, int stat, void* work, size_t work_bytes, double* out, int64_t* out_counts,
              int32_t* out_status, void* stream) {
    if (!frames || !shapes) return fail(SPX_E_ARG, "null table (frames, shapes)");
    if (!out || !out_counts || !out_status) return fail(SPX_E_ARG, "null output");
    if (nframes < 1 || nframes > spx::kSkyMaxFrames) return fail(SPX_E_ARG, "nframes must be 1..128");
    if (!(lsigma > 0.0) || !(lsigma - lsigma == 0.0) || !(usigma > 0.0) || !(usigma - usigma == 0.0))
        return fail(SPX_E_ARG, "lsigma and usigma must be positive and finite");
    if (max_iters < 0) return fail(SPX_E_ARG, "max_iters must not be negative");
    if (stat != SPX_SKY_MEDIAN && stat != SPX_SKY_MEAN && stat != SPX_SKY_MODE)
        return fail(SPX_E_ARG, "stat must be SPX_SKY_MEDIAN, SPX_SKY_MEAN or SPX_SKY_MODE");
    if (lower > upper) return fail(SPX_E_ARG, "lower must not exceed upper");
    if (max_iters > 1000) return fail(SPX_E_ARG, "max_iters must not exceed 1000");
    const size_t need = (size_t)nframes * spx::kSkyFrameBytes;
    if (!work || work_bytes < need)
        return fail(SPX_E_WORKSPACE, "workspace missing or smaller than spx_sky_workspace_bytes(nframes)");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const T* const* fr = reinterpret_cast<const T* const*>(frames);
    const T* const* wt = reinterpret_cast<const T* const*>(weights);
    int gpf = 2048 / nframes;                       // hist workgroups per frame: free (integer sums)
    gpf = gpf < 16 ? 16 : (gpf > 512 ? 512 : gpf);
    SPX_HIP(hipMemsetAsync(work, 0, need, s));
    hipError_t err = hipSuccess;
    spx::host::sky_stats_launch(spx::SkyKey<T>::digits, max_iters, [&](int kind, int pass, int round) {
        if (err != hipSuccess) return;
        switch (kind) {
        case 0:
            hipLaunchKernelGGL(spx::sky_init_kernel, dim3(1), dim3(256), 0, s, frames, shapes, nframes, lower, upper,
                               work);
            break;
        case 1:
            hipLaunchKernelGGL(spx::sky_hist_kernel<T>, dim3((unsigned)(nframes * gpf)), dim3(256),
                               spx::kSkyHistLdsBytes, s, fr, wt, masks, shapes, nframes, gpf, pass, work);
            break;
        case 2:
            hipLaunchKernelGGL(spx::sky_select_kernel<T>, dim3((unsigned)nframes), dim3(256), spx::kSkySelectLdsBytes,
                               s, nframes, pass, round, work);
            break;
        case 3:
            hipLaunchKernelGGL(spx::sky_moments_kernel<T>, dim3((unsigned)(nframes * spx::kSkyMomentGrid)), dim3(256),
                               spx::kSkyMomentLdsBytes, s, fr, wt, masks, shapes, nframes, work);
            break;
        case 4:
            hipLaunchKernelGGL(spx::sky_finish_kernel, dim3(1), dim3(256), 0, s, nframes, round, max_iters, lsigma,
                               usigma, work);
            break;
        default:
            hipLaunchKernelGGL(spx::sky_output_kernel, dim3(1), dim3(256), 0, s, nframes, stat, (const void*)work, out,
                               reinterpret_cast<long long*>(out_counts), out_status);
        }
        err = hipGetLastError();
    });
    SPX_HIP(err);
    return 0;
}
}  // namespace

extern "C" {

size_t spx_sky_workspace_bytes(int nframes) {
    if (nframes < 1 || nframes > spx::kSkyMaxFrames) return 0;
    return (size_t)nframes * spx::kSkyFrameBytes;
}
int spx_sky_stats_f32(const void* const* frames, const void* const* weights, const uint8_t* const* masks,
                      const int32_t* shapes, int nframes, double lower, double upper, double lsigma, double usigma,
                      int max_iters, int stat, void* work, size_t work_bytes, double* out, int64_t* out_counts,
                      int32_t* out_status, void* stream) {
    return sky_stats<float>(frames, weights, masks, shapes, nframes, lower, upper, lsigma, usigma, max_iters, stat,
                            work, work_bytes, out, out_counts, out_status, stream);
}
int spx_sky_stats_f64(const void* const* frames, const void* const* weights, const uint8_t* const* masks,
                      const int32_t* shapes, int nframes, double lower, double upper, double lsigma, double usigma,
                      int max_iters, int stat, void* work, size_t work_bytes, double* out, int64_t* out_counts,
                      int32_t* out_status, void* stream) {
    return sky_stats<double>(frames, weights, masks, shapes, nframes, lower, upper, lsigma, usigma, max_iters, stat,
                             work, work_bytes, out, out_counts, out_status, stream);
}

}  // extern "C"
