// TEST INFRASTRUCTURE ONLY: the kernels of spx_minmed_kernels.h on CPU threads (spx_rt_emu.h), launched as
// spx_capi.hip launches them (the same tile counts, the same dynamic-LDS sizes), for tests/test_minmed_cpu.py.  It
// includes emu_crreject.cpp, so the one library also holds the drizzle's, the median's and the comparison's harness.
// Built on its own (one object, the Makefile's emu compiler and flags).  `grid` caps the number of workgroups.
#include "emu_crreject.cpp"

#include "spx_minmed_kernels.h"

namespace {
template <typename T>
int mm_minmed(const T* const* frames, const T* const* weights, const uint8_t* const* masks, const int32_t* shapes,
              const double* maps, const uint8_t* active, int nframes, double pixfrac, int kernel, int nlow, int nhigh,
              const double* table, double nsigma1, double nsigma2, int grow, int out_ny, int out_nx, float* md,
              float* lo, uint8_t* bits, float* med, uint8_t* nmed, uint8_t* minmed, int grid) {
    std::vector<DrizzleRow> rows;
    int nactive = 0;
    if (const int rc = pack_rows(frames, weights, masks, shapes, maps, active, nframes, pixfrac, kernel, rows, &nactive))
        return rc;
    if (nactive < 1 || grow < 0 || grow > kMmMaxGrow) return -1;
    const int64_t tiles = (int64_t)((out_nx + kDrzTileW - 1) / kDrzTileW) * ((out_ny + kDrzTileH - 1) / kDrzTileH);
    const DrizzleRow* r = rows.data();
    rt::launch(grid > 0 && grid < tiles ? grid : tiles, 256, [&] {
        drizzle_minmed_kernel<T>(r, nframes, nactive, kernel, nlow, nhigh, table, nsigma1, nsigma2, out_ny, out_nx, md,
                                 lo, bits, nmed);
    }, drizzle_median_lds_bytes(nactive));
    rt::launch(grid > 0 && grid < tiles ? grid : tiles, 256, [&] {
        minmed_grow_kernel(md, lo, bits, grow, out_ny, out_nx, med, minmed);
    }, kMmGrowLdsBytes);
    return 0;
}

template <typename T>
int mm_cr_grow(const T* const* frames, const T* const* weights, const uint8_t* const* masks, const int32_t* shapes,
               const double* maps, const uint8_t* active, int nframes, double pixfrac, int kernel, int frame,
               const float* med, const uint8_t* nmed, int out_ny, int out_nx, double rms_scalar, const T* rms_map,
               const uint8_t* seed, int g, int c, int ctedir, uint8_t* crmask, T* clean, int grid) {
    std::vector<DrizzleRow> rows;
    int nactive = 0;
    if (const int rc = pack_rows(frames, weights, masks, shapes, maps, active, nframes, pixfrac, kernel, rows, &nactive))
        return rc;
    if (frame < 0 || frame >= nframes || out_ny < kCrMinOut || out_nx < kCrMinOut) return -1;
    if (g < 1 || g > 2 * kCrGrowMaxHalf + 1 || !(g & 1) || c < 0 || c > kCrGrowMaxCte || ctedir < -1 || ctedir > 1)
        return -1;
    const int fny = shapes[2 * frame], fnx = shapes[2 * frame + 1];
    const int64_t tiles = (int64_t)((fnx + kDrzTileW - 1) / kDrzTileW) * ((fny + kDrzTileH - 1) / kDrzTileH);
    const DrizzleRow* r = rows.data();
    rt::launch(grid > 0 && grid < tiles ? grid : tiles, 256, [&] {
        drizzle_cr_grow_kernel<T>(r, frame, med, nmed, out_ny, out_nx, rms_scalar, rms_map, seed, g, c, ctedir, crmask,
                                  clean);
    }, kCrGrowLdsBytes);
    return 0;
}
}  // namespace

#define EMUZ_MM(SUFFIX, T)                                                                                            \
    extern "C" int emuz_mm_minmed_##SUFFIX(const T* const* frames, const T* const* weights,                           \
                                           const uint8_t* const* masks, const int32_t* shapes, const double* maps,    \
                                           const uint8_t* active, int nframes, double pixfrac, int kernel, int nlow,   \
                                           int nhigh, const double* table, double nsigma1, double nsigma2, int grow,   \
                                           int out_ny, int out_nx, float* md, float* lo, uint8_t* bits, float* med,    \
                                           uint8_t* nmed, uint8_t* minmed, int grid) {                                 \
        return mm_minmed<T>(frames, weights, masks, shapes, maps, active, nframes, pixfrac, kernel, nlow, nhigh, table, \
                            nsigma1, nsigma2, grow, out_ny, out_nx, md, lo, bits, med, nmed, minmed, grid);            \
    }                                                                                                                  \
    extern "C" int emuz_mm_cr_grow_##SUFFIX(const T* const* frames, const T* const* weights,                          \
                                            const uint8_t* const* masks, const int32_t* shapes, const double* maps,   \
                                            const uint8_t* active, int nframes, double pixfrac, int kernel, int frame, \
                                            const float* med, const uint8_t* nmed, int out_ny, int out_nx,            \
                                            double rms_scalar, const T* rms_map, const uint8_t* seed, int g, int c,    \
                                            int ctedir, uint8_t* crmask, T* clean, int grid) {                         \
        return mm_cr_grow<T>(frames, weights, masks, shapes, maps, active, nframes, pixfrac, kernel, frame, med, nmed, \
                             out_ny, out_nx, rms_scalar, rms_map, seed, g, c, ctedir, crmask, clean, grid);            \
    }
EMUZ_MM(f32, float)
EMUZ_MM(f64, double)
