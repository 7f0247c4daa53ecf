// TEST INFRASTRUCTURE ONLY: the deblending kernels (spx_deblend_kernels.h) on CPU threads (spx_rt_emu.h),
// launched in the order and with the LDS sizes of spx_capi.hip's deblend_labels, for tests/test_deblend_cpu.py.
// Built on its own (one object, the Makefile's emu compiler and flags) so the other harnesses stay as they are.
// The harness runs the workgroups of a launch ONE AFTER ANOTHER with real threads inside a workgroup: it proves
// the kernels' logic, index arithmetic and the barriers between the phases of a level.  A parent never depends
// on another workgroup, so there is nothing between workgroups left to prove for the parent kernel.
#include "spx_rt_emu.h"

namespace spx {
namespace rt {
// twins of the primitives spx_rt_hip.h has for the union-find and gained for the deblending
SPX_DEVICE int atomic_min_ret_i32(int* p, int v) {
    int o = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < o && !__atomic_compare_exchange_n(p, &o, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return o;
}
SPX_DEVICE int atomic_load_i32(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
SPX_DEVICE void atomic_accum_u64(unsigned long long* p, unsigned long long v) {
    __atomic_fetch_add(p, v, __ATOMIC_RELAXED);
}
SPX_DEVICE void atomic_or_i32(int* p, int v) { __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
}  // namespace rt
}  // namespace spx

#include "spx_kernels.h"
#include "spx_aux_kernels.h"
#include "spx_detect_kernels.h"
#include "spx_deblend_kernels.h"

using namespace spx;

namespace {
int64_t cap(int64_t blocks, int64_t most) { return blocks < 1 ? 1 : (blocks < most ? blocks : most); }

// lds_pixels / wave_pixels: the class limits (kDebLdsPixels / kDebWavePixels in the library); a test may lower
// lds_pixels to send a small parent through the workspace path
template <typename T>
int deblend(const T* frame, const uint8_t* bad, const T* filt, int fky, int fkx, int fny, int fnx,
            const int32_t* labels, int nlabels, const int32_t* boxes, int conn, int min_area, int nlev, double contrast,
            int mode, int32_t* out_labels, int32_t* out_parent, int32_t* out_dflags, int max_out, int32_t* out_nlabels,
            int grid, int lds_pixels) {
    if (!filt) fky = fkx = 1;
    const int npix = fny * fnx;
    const int64_t nchunks = ((int64_t)npix + kDetChunk - 1) / kDetChunk;
    std::vector<int32_t> R(npix, 0), cnt(npix, -7), sums(nchunks, -7), pflag(nlabels + 1, 0);
    int32_t status = 0;
    const int64_t most = npix < kDebMaxBoxPixels ? npix : kDebMaxBoxPixels;
    const size_t slot_bytes = ((size_t)most * kDebBytesPerPixel + 255) / 256 * 256;
    const int nslots = (int)cap(nlabels < kDebSlots ? nlabels : kDebSlots, grid);
    std::vector<unsigned long long> slots((slot_bytes * nslots + 7) / 8, 0xCDCDCDCDCDCDCDCDull);
    unsigned char* sl = reinterpret_cast<unsigned char*>(slots.data());
    const int wave_pixels = lds_pixels < kDebWavePixels ? lds_pixels : kDebWavePixels;
    if (nlabels > 0) {
        rt::launch(cap(nlabels, grid), 64, [&] {
            deblend_parents_kernel<T, 64, false>(frame, bad, filt, fky, fkx, fny, fnx, labels, nlabels, boxes, conn,
                                                 min_area, nlev, contrast, mode, 0, wave_pixels, sl, slot_bytes,
                                                 R.data(), cnt.data(), pflag.data(), &status);
        }, deb_lds_bytes(wave_pixels));
        const int mid[3] = {wave_pixels, kDebMidPixels < lds_pixels ? kDebMidPixels : lds_pixels, lds_pixels};
        for (int c = 0; c < 2 && npix > mid[c]; ++c) {
            if (mid[c + 1] <= mid[c]) continue;
            rt::launch(cap(nlabels, grid), 256, [&] {
                deblend_parents_kernel<T, 256, false>(frame, bad, filt, fky, fkx, fny, fnx, labels, nlabels, boxes,
                                                      conn, min_area, nlev, contrast, mode, mid[c] + 1, mid[c + 1], sl,
                                                      slot_bytes, R.data(), cnt.data(), pflag.data(), &status);
            }, deb_lds_bytes(mid[c + 1]));
        }
        if (npix > lds_pixels)
            rt::launch(nslots, kDebWsThreads, [&] {
                deblend_parents_kernel<T, kDebWsThreads, true>(frame, bad, filt, fky, fkx, fny, fnx, labels, nlabels,
                                                               boxes, conn, min_area, nlev, contrast, mode,
                                                               lds_pixels + 1, kDebMaxBoxPixels, sl, slot_bytes,
                                                               R.data(), cnt.data(), pflag.data(), &status);
            }, deb_lds_bytes(0));
    }
    rt::launch(cap(nchunks, grid), 256, [&] {
        detect_flag_count_kernel(R.data(), cnt.data(), npix, 1, sums.data());
    }, kDetScanLdsBytes);
    rt::launch(1, 256, [&] { detect_scan_blocks_kernel(sums.data(), nchunks, &status, out_nlabels); }, kDetScanLdsBytes);
    rt::launch(cap(nchunks, grid), 256, [&] {
        detect_assign_kernel(R.data(), cnt.data(), npix, 1, sums.data());
    }, kDetScanLdsBytes);
    rt::launch(cap(((int64_t)npix + 255) / 256, grid), 256, [&] {
        detect_relabel_kernel(R.data(), cnt.data(), npix, out_labels);
    }, 0);
    rt::launch(cap(((int64_t)npix + 255) / 256, grid), 256, [&] {
        deblend_table_kernel(R.data(), cnt.data(), labels, pflag.data(), npix, nlabels, max_out, out_parent,
                             out_dflags);
    }, 0);
    return 0;
}
}  // namespace

extern "C" int emub_lds_pixels() { return kDebLdsPixels; }
extern "C" int emub_wave_pixels() { return kDebWavePixels; }
extern "C" int emub_max_box_pixels() { return kDebMaxBoxPixels; }

extern "C" int emub_deblend_f32(const float* frame, const uint8_t* bad, const float* filt, int fky, int fkx, int fny,
                                int fnx, const int32_t* labels, int nlabels, const int32_t* boxes, int conn,
                                int min_area, int nlev, double contrast, int mode, int32_t* out_labels,
                                int32_t* out_parent, int32_t* out_dflags, int max_out, int32_t* out_nlabels, int grid,
                                int lds_pixels) {
    return deblend<float>(frame, bad, filt, fky, fkx, fny, fnx, labels, nlabels, boxes, conn, min_area, nlev, contrast,
                          mode, out_labels, out_parent, out_dflags, max_out, out_nlabels, grid, lds_pixels);
}
extern "C" int emub_deblend_f64(const double* frame, const uint8_t* bad, const double* filt, int fky, int fkx, int fny,
                                int fnx, const int32_t* labels, int nlabels, const int32_t* boxes, int conn,
                                int min_area, int nlev, double contrast, int mode, int32_t* out_labels,
                                int32_t* out_parent, int32_t* out_dflags, int max_out, int32_t* out_nlabels, int grid,
                                int lds_pixels) {
    return deblend<double>(frame, bad, filt, fky, fkx, fny, fnx, labels, nlabels, boxes, conn, min_area, nlev, contrast,
                           mode, out_labels, out_parent, out_dflags, max_out, out_nlabels, grid, lds_pixels);
}
