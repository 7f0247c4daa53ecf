// TEST INFRASTRUCTURE ONLY: the catalog path's float64 gathers and blots (spx_aux_kernels.h) on CPU threads
// (spx_rt_emu.h), next to their float32 instances, for tests/test_catalog_f64_cpu.py.  Built on its own
// (one object, the Makefile's emu compiler and flags) so the main harness stays as it is.
#include "spx_rt_emu.h"
#include "spx_kernels.h"
#include "spx_aux_kernels.h"

using namespace spx;

extern "C" int emu64_gather(const double* frame, const uint8_t* fmask, int fny, int fnx, const int32_t* boxes,
                            int64_t nbatch, int tny, int tnx, double fill, double* tiles, const int32_t* seg,
                            const int32_t* ids) {
    const int64_t blocks = (nbatch * tny * tnx + 255) / 256;
    rt::launch(blocks < 8 ? blocks : 8, 256, [&] {
        gather_cutouts_kernel(frame, fmask, fny, fnx, boxes, nbatch, tny, tnx, fill, tiles, seg, ids);
    }, 0);
    return 0;
}

extern "C" int emu64_gather_var(const double* frame, const uint8_t* fmask, int fny, int fnx, const int32_t* boxes,
                                int64_t nbatch, const int64_t* off, double fill, double* out, const int32_t* seg,
                                const int32_t* ids) {
    rt::launch(nbatch < 3 ? nbatch : 3, 256, [&] {
        gather_cutouts_var_kernel(frame, fmask, fny, fnx, boxes, nbatch, off, fill, out, seg, ids);
    }, 0);
    return 0;
}

// the blots of one catalog, stored as float32 (spx_blot4_var_f32) or float64 (spx_blot4_var_to_f64)
extern "C" int emu64_blot4_var_f32(const float* src, const int64_t* src_off, const int32_t* src_shp, int64_t nbatch,
                                   const double* map, int degree, const float* gain, const int64_t* dst_off,
                                   const int32_t* dst_shp, float* im4) {
    rt::launch(nbatch < 3 ? nbatch : 3, 256, [&] {
        blot4_var_kernel(src, src_off, src_shp, nbatch, map, degree, gain, dst_off, dst_shp, im4);
    }, 0);
    return 0;
}

extern "C" int emu64_blot4_var_to_f64(const float* src, const int64_t* src_off, const int32_t* src_shp,
                                      int64_t nbatch, const double* map, int degree, const float* gain,
                                      const int64_t* dst_off, const int32_t* dst_shp, double* im4) {
    rt::launch(nbatch < 3 ? nbatch : 3, 256, [&] {
        blot4_var_kernel(src, src_off, src_shp, nbatch, map, degree, gain, dst_off, dst_shp, im4);
    }, 0);
    return 0;
}
