// TEST INFRASTRUCTURE ONLY: the polynomial-map drizzle kernel (spx_drizzle_poly_kernels.h) on CPU threads
// (spx_rt_emu.h), with rows packed by the library's own host::drizzle_poly_pack_row and launched as spx_capi.hip
// launches it, for tests/test_drizzle_poly_cpu.py.  Built on its own (one object, the Makefile's emu compiler and
// flags).  The workgroups of a launch run ONE AFTER ANOTHER with real threads inside a workgroup; `grid` caps the
// number of workgroups.
#include "spx_rt_emu.h"

#include "spx_drizzle_kernels.h"
#include "spx_drizzle_poly_kernels.h"

using namespace spx;

namespace {
// 0, or the code of host::drizzle_poly_pack_row for the first frame it refuses (nothing is written then)
template <typename T>
int drizzle_poly(const T* const* frames, const T* const* weights, const uint8_t* const* masks, const int32_t* shapes,
                 const double* coef, const int32_t* degree, const double* center, const uint8_t* active, int nframes,
                 double pixfrac, int kernel, double fill, int out_ny, int out_nx, T* sci, float* wht, int32_t* ctx,
                 int grid) {
    std::vector<DrizzlePolyRow> rows((size_t)nframes);
    for (int k = 0; k < nframes; ++k) {
        const int rc = host::drizzle_poly_pack_row(frames[k], weights ? weights[k] : nullptr,
                                                   masks ? masks[k] : nullptr, shapes[2 * k], shapes[2 * k + 1],
                                                   active ? active[k] : 1, coef + (size_t)k * 2 * kDrzPolyTerms,
                                                   degree[k], center + 2 * k, pixfrac, kernel, &rows[(size_t)k]);
        if (rc) return rc;
    }
    const int64_t tiles = (int64_t)((out_nx + kDrzTileW - 1) / kDrzTileW) * ((out_ny + kDrzTileH - 1) / kDrzTileH);
    const DrizzlePolyRow* r = rows.data();
    rt::launch(grid > 0 && grid < tiles ? grid : tiles, 256, [&] {
        drizzle_poly_kernel<T>(r, nframes, kernel, fill, out_ny, out_nx, sci, wht, ctx);
    }, 0);
    return 0;
}
}  // namespace

extern "C" int emuz_drizzle_poly_f32(const float* const* frames, const float* const* weights,
                                     const uint8_t* const* masks, const int32_t* shapes, const double* coef,
                                     const int32_t* degree, const double* center, const uint8_t* active, int nframes,
                                     double pixfrac, int kernel, double fill, int out_ny, int out_nx, float* sci,
                                     float* wht, int32_t* ctx, int grid) {
    return drizzle_poly<float>(frames, weights, masks, shapes, coef, degree, center, active, nframes, pixfrac, kernel,
                               fill, out_ny, out_nx, sci, wht, ctx, grid);
}
extern "C" int emuz_drizzle_poly_f64(const double* const* frames, const double* const* weights,
                                     const uint8_t* const* masks, const int32_t* shapes, const double* coef,
                                     const int32_t* degree, const double* center, const uint8_t* active, int nframes,
                                     double pixfrac, int kernel, double fill, int out_ny, int out_nx, double* sci,
                                     float* wht, int32_t* ctx, int grid) {
    return drizzle_poly<double>(frames, weights, masks, shapes, coef, degree, center, active, nframes, pixfrac, kernel,
                                fill, out_ny, out_nx, sci, wht, ctx, grid);
}
