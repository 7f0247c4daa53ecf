// TEST INFRASTRUCTURE ONLY: the source-finding kernels (spx_detect_kernels.h) on CPU threads (spx_rt_emu.h),
// launched in the order and with the LDS sizes of spx_capi.hip's detect_label / measure_labels, for
// tests/test_detect_cpu.py.  Built on its own (one object, the Makefile's emu compiler and flags) so the main
// harness stays as it is.
// The harness runs the workgroups of a launch ONE AFTER ANOTHER, with real threads inside a workgroup: it
// proves the kernels' logic, index arithmetic and intra-workgroup synchronisation (the LDS union-find runs on
// truly concurrent threads), NOT the races between workgroups that the global merge meets on a GPU
// (tests/test_gpu_detect.py covers those).
#include "spx_rt_emu.h"

namespace spx {
namespace rt {
// twins of the two primitives spx_rt_hip.h gained for the union-find
SPX_DEVICE int atomic_min_ret_i32(int* p, int v) {
    int o = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < o && !__atomic_compare_exchange_n(p, &o, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return o;
}
SPX_DEVICE int atomic_load_i32(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
}  // namespace rt
}  // namespace spx

#include "spx_kernels.h"
#include "spx_aux_kernels.h"
#include "spx_detect_kernels.h"

using namespace spx;

namespace {
int64_t cap(int64_t blocks, int64_t most) { return blocks < 1 ? 1 : (blocks < most ? blocks : most); }

template <typename T>
int detect_label(const T* frame, const uint8_t* bad, T thr, const float* thr_map, const T* filt, int fky, int fkx,
                 int fny, int fnx, int conn, int min_area, int32_t* labels, int32_t* nlabels, int grid) {
    if (!filt) fky = fkx = 1;
    const int npix = fny * fnx;
    const int64_t nchunks = ((int64_t)npix + kDetChunk - 1) / kDetChunk;
    std::vector<int32_t> R(npix, -7), cnt(npix, -7), sums(nchunks, -7);
    int32_t status = 0;
    const int64_t ntiles = (int64_t)((fnx + kDetTW - 1) / kDetTW) * ((fny + kDetTH - 1) / kDetTH);
    rt::launch(cap(ntiles, grid), 256, [&] {
        detect_tile_kernel<T>(frame, bad, thr, thr_map, filt, fky, fkx, fny, fnx, conn, labels, cnt.data(), &status);
    }, det_tile_lds_bytes(sizeof(T), fky, fkx));
    const int64_t nborder = (int64_t)((fny + kDetTH - 1) / kDetTH - 1) * fnx +
                            2 * (int64_t)((fnx + kDetTW - 1) / kDetTW - 1) * fny;
    if (nborder > 0)
        rt::launch(cap((nborder + 255) / 256, grid), 256, [&] {
            detect_border_kernel(labels, fny, fnx, conn, &status);
        }, 0);
    rt::launch(cap(((int64_t)npix + 1023) / 1024, grid), 256, [&] {
        detect_compress_kernel(labels, npix, R.data(), cnt.data(), &status);
    }, 0);
    rt::launch(cap(nchunks, grid), 256, [&] {
        detect_flag_count_kernel(R.data(), cnt.data(), npix, min_area, sums.data());
    }, kDetScanLdsBytes);
    rt::launch(1, 256, [&] { detect_scan_blocks_kernel(sums.data(), nchunks, &status, nlabels); }, kDetScanLdsBytes);
    rt::launch(cap(nchunks, grid), 256, [&] {
        detect_assign_kernel(R.data(), cnt.data(), npix, min_area, sums.data());
    }, kDetScanLdsBytes);
    rt::launch(cap(((int64_t)npix + 255) / 256, grid), 256, [&] {
        detect_relabel_kernel(R.data(), cnt.data(), npix, labels);
    }, 0);
    return 0;
}

template <typename T>
int measure(const T* frame, const uint8_t* bad, double bkg, const T* bkg_map, const int32_t* labels, int fny, int fnx,
            int nlabels, const int32_t* boxes, double* table, int32_t* flags, int grid) {
    if (nlabels == 0) return 0;
    rt::launch(cap(nlabels, grid), 256, [&] {
        measure_labels_kernel<T>(frame, bad, bkg, bkg_map, labels, fny, fnx, nlabels, boxes, table, flags);
    }, kMeasureLdsBytes);
    return 0;
}
}  // namespace

extern "C" int emud_detect_label_f32(const float* frame, const uint8_t* bad, float thr, const float* thr_map,
                                     const float* filt, int fky, int fkx, int fny, int fnx, int conn, int min_area,
                                     int32_t* labels, int32_t* nlabels, int grid) {
    return detect_label<float>(frame, bad, thr, thr_map, filt, fky, fkx, fny, fnx, conn, min_area, labels, nlabels,
                               grid);
}
extern "C" int emud_detect_label_f64(const double* frame, const uint8_t* bad, double thr, const float* thr_map,
                                     const double* filt, int fky, int fkx, int fny, int fnx, int conn, int min_area,
                                     int32_t* labels, int32_t* nlabels, int grid) {
    return detect_label<double>(frame, bad, thr, thr_map, filt, fky, fkx, fny, fnx, conn, min_area, labels, nlabels,
                                grid);
}

// spx_label_bboxes_i32 as spx_capi.hip launches it
extern "C" int emud_label_bboxes(const int32_t* seg, int fny, int fnx, int max_label, int32_t* boxes,
                                 int32_t* counts, int grid) {
    const int nl = max_label + 1;
    rt::launch((nl + 255) / 256, 256, [&] { label_bbox_init_kernel(boxes, counts, nl); }, 0);
    const int64_t total = (int64_t)fny * ((fnx + 3) / 4);
    rt::launch(cap((total + 255) / 256, grid), 256, [&] {
        label_bbox_kernel(seg, fny, fnx, max_label, boxes, counts);
    }, 0);
    return 0;
}

extern "C" int emud_measure_f32(const float* frame, const uint8_t* bad, double bkg, const float* bkg_map,
                                const int32_t* labels, int fny, int fnx, int nlabels, const int32_t* boxes,
                                double* table, int32_t* flags, int grid) {
    return measure<float>(frame, bad, bkg, bkg_map, labels, fny, fnx, nlabels, boxes, table, flags, grid);
}
extern "C" int emud_measure_f64(const double* frame, const uint8_t* bad, double bkg, const double* bkg_map,
                                const int32_t* labels, int fny, int fnx, int nlabels, const int32_t* boxes,
                                double* table, int32_t* flags, int grid) {
    return measure<double>(frame, bad, bkg, bkg_map, labels, fny, fnx, nlabels, boxes, table, flags, grid);
}
