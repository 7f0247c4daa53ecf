// TEST INFRASTRUCTURE ONLY: the cosmic-ray kernels (spx_crreject_kernels.h) on CPU threads (spx_rt_emu.h), with rows
// packed by the library's own host::drizzle_pack_row and launched as spx_capi.hip launches them (the same tile
// counts, the same dynamic-LDS sizes, host::cr_params), for tests/test_crreject_cpu.py.  It includes emu_drizzle.cpp,
// so the one library also holds emuz_drizzle_f32 / _f64 for the single-frame runs the median is pinned with.  Built
// on its own (one object, the Makefile's emu compiler and flags).  `grid` caps the number of workgroups.
#include "spx_rt_emu.h"

#include "spx_kernels.h"
#include "spx_aux_kernels.h"

#include "emu_drizzle.cpp"

#include "spx_crreject_kernels.h"

namespace {
template <typename T>
int pack_rows(const T* const* frames, const T* const* weights, const uint8_t* const* masks, const int32_t* shapes,
              const double* maps, const uint8_t* active, int nframes, double pixfrac, int kernel,
              std::vector<DrizzleRow>& rows, int* nactive) {
    rows.resize((size_t)nframes);
    *nactive = 0;
    for (int k = 0; k < nframes; ++k) {
        const int rc = host::drizzle_pack_row(frames[k], weights ? weights[k] : nullptr, masks ? masks[k] : nullptr,
                                              shapes[2 * k], shapes[2 * k + 1], active ? active[k] : 1, maps + 6 * k,
                                              pixfrac, kernel, &rows[(size_t)k]);
        if (rc) return rc;
        *nactive += rows[(size_t)k].active;
    }
    return 0;
}

template <typename T>
int crr_median(const T* const* frames, const T* const* weights, const uint8_t* const* masks, const int32_t* shapes,
               const double* maps, const uint8_t* active, int nframes, double pixfrac, int kernel, int nlow, int nhigh,
               int out_ny, int out_nx, float* med, uint8_t* nmed, int grid) {
    std::vector<DrizzleRow> rows;
    int nactive = 0;
    if (const int rc = pack_rows(frames, weights, masks, shapes, maps, active, nframes, pixfrac, kernel, rows, &nactive))
        return rc;
    if (nactive < 1) return -1;
    const int64_t tiles = (int64_t)((out_nx + kDrzTileW - 1) / kDrzTileW) * ((out_ny + kDrzTileH - 1) / kDrzTileH);
    const DrizzleRow* r = rows.data();
    rt::launch(grid > 0 && grid < tiles ? grid : tiles, 256, [&] {
        drizzle_median_kernel<T>(r, nframes, nactive, kernel, nlow, nhigh, out_ny, out_nx, med, nmed);
    }, drizzle_median_lds_bytes(nactive));
    return 0;
}

template <typename T>
int crr_cr(const T* const* frames, const T* const* weights, const uint8_t* const* masks, const int32_t* shapes,
           const double* maps, const uint8_t* active, int nframes, double pixfrac, int kernel, int frame,
           const float* med, const uint8_t* nmed, int out_ny, int out_nx, double rms_scalar, const T* rms_map,
           double sky, double gain, double snr1, double snr2, double scale1, double scale2, uint8_t* crmask, T* clean,
           int grid) {
    std::vector<DrizzleRow> rows;
    int nactive = 0;
    if (const int rc = pack_rows(frames, weights, masks, shapes, maps, active, nframes, pixfrac, kernel, rows, &nactive))
        return rc;
    if (frame < 0 || frame >= nframes || out_ny < kCrMinOut || out_nx < kCrMinOut) return -1;
    const int fny = shapes[2 * frame], fnx = shapes[2 * frame + 1];
    const int64_t tiles = (int64_t)((fnx + kDrzTileW - 1) / kDrzTileW) * ((fny + kDrzTileH - 1) / kDrzTileH);
    const CrParams c = host::cr_params(rms_scalar, sky, gain, snr1, snr2, scale1, scale2);
    const DrizzleRow* r = rows.data();
    rt::launch(grid > 0 && grid < tiles ? grid : tiles, 256, [&] {
        drizzle_cr_kernel<T>(r, frame, med, nmed, out_ny, out_nx, rms_map, c, crmask, clean);
    }, kCrLdsBytes);
    return 0;
}
}  // namespace

#define EMUZ_CRR(SUFFIX, T)                                                                                           \
    extern "C" int emuz_crr_median_##SUFFIX(const T* const* frames, const T* const* weights,                          \
                                            const uint8_t* const* masks, const int32_t* shapes, const double* maps,   \
                                            const uint8_t* active, int nframes, double pixfrac, int kernel, int nlow,  \
                                            int nhigh, int out_ny, int out_nx, float* med, uint8_t* nmed, int grid) { \
        return crr_median<T>(frames, weights, masks, shapes, maps, active, nframes, pixfrac, kernel, nlow, nhigh,      \
                             out_ny, out_nx, med, nmed, grid);                                                         \
    }                                                                                                                  \
    extern "C" int emuz_crr_cr_##SUFFIX(const T* const* frames, const T* const* weights, const uint8_t* const* masks,  \
                                        const int32_t* shapes, const double* maps, const uint8_t* active, int nframes, \
                                        double pixfrac, int kernel, int frame, const float* med, const uint8_t* nmed,  \
                                        int out_ny, int out_nx, double rms_scalar, const T* rms_map, double sky,       \
                                        double gain, double snr1, double snr2, double scale1, double scale2,           \
                                        uint8_t* crmask, T* clean, int grid) {                                         \
        return crr_cr<T>(frames, weights, masks, shapes, maps, active, nframes, pixfrac, kernel, frame, med, nmed,     \
                         out_ny, out_nx, rms_scalar, rms_map, sky, gain, snr1, snr2, scale1, scale2, crmask, clean,    \
                         grid);                                                                                        \
    }
EMUZ_CRR(f32, float)
EMUZ_CRR(f64, double)
