// TEST INFRASTRUCTURE ONLY: the whole-frame statistics kernels (spx_sky_kernels.h) on CPU threads (spx_rt_emu.h),
// launched as spx_capi.hip launches them: the same host::sky_stats_launch sequence, the same dynamic-LDS sizes, the
// moment grid of the header.  Only the hist kernel's workgroups per frame differ (`gpf`, default 2; the library
// takes 16 .. 512): its sums are integers, and tests/test_sky_cpu.py checks that the results do not depend on it.
// Built on its own (one object, the Makefile's emu compiler and flags).  All tables are host memory here.
#include "spx_rt_emu.h"

#include "spx_sky_kernels.h"

namespace {
using namespace spx;

template <typename T>
int sky_stats(const void* const* frames, const void* const* weights, const uint8_t* const* masks,
              const int32_t* shapes, int nframes, double lower, double upper, double lsigma, double usigma,
              int max_iters, int stat, double* out, long long* out_counts, int32_t* out_status, int gpf) {
    if (nframes < 1 || nframes > kSkyMaxFrames || max_iters < 0) return -1;
    if (gpf < 1) gpf = 2;
    std::vector<unsigned char> workv((size_t)nframes * kSkyFrameBytes + 16, 0);
    void* work = workv.data() + (16 - reinterpret_cast<uintptr_t>(workv.data()) % 16) % 16;
    const T* const* fr = reinterpret_cast<const T* const*>(frames);
    const T* const* wt = reinterpret_cast<const T* const*>(weights);
    host::sky_stats_launch(SkyKey<T>::digits, max_iters, [&](int kind, int pass, int round) {
        switch (kind) {
        case 0:
            rt::launch(1, 256, [&] { sky_init_kernel(frames, shapes, nframes, lower, upper, work); }, 0);
            break;
        case 1:
            rt::launch((int64_t)nframes * gpf, 256,
                       [&] { sky_hist_kernel<T>(fr, wt, masks, shapes, nframes, gpf, pass, work); }, kSkyHistLdsBytes);
            break;
        case 2:
            rt::launch(nframes, 256, [&] { sky_select_kernel<T>(nframes, pass, round, work); }, kSkySelectLdsBytes);
            break;
        case 3:
            rt::launch((int64_t)nframes * kSkyMomentGrid, 256,
                       [&] { sky_moments_kernel<T>(fr, wt, masks, shapes, nframes, work); }, kSkyMomentLdsBytes);
            break;
        case 4:
            rt::launch(1, 256, [&] { sky_finish_kernel(nframes, round, max_iters, lsigma, usigma, work); }, 0);
            break;
        default:
            rt::launch(1, 256, [&] { sky_output_kernel(nframes, stat, work, out, out_counts, out_status); }, 0);
        }
    });
    return 0;
}
}  // namespace

extern "C" int emus_sky_stats_f32(const void* const* frames, const void* const* weights, const uint8_t* const* masks,
                                  const int32_t* shapes, int nframes, double lower, double upper, double lsigma,
                                  double usigma, int max_iters, int stat, double* out, long long* out_counts,
                                  int32_t* out_status, int gpf) {
    return sky_stats<float>(frames, weights, masks, shapes, nframes, lower, upper, lsigma, usigma, max_iters, stat,
                            out, out_counts, out_status, gpf);
}
extern "C" int emus_sky_stats_f64(const void* const* frames, const void* const* weights, const uint8_t* const* masks,
                                  const int32_t* shapes, int nframes, double lower, double upper, double lsigma,
                                  double usigma, int max_iters, int stat, double* out, long long* out_counts,
                                  int32_t* out_status, int gpf) {
    return sky_stats<double>(frames, weights, masks, shapes, nframes, lower, upper, lsigma, usigma, max_iters, stat,
                             out, out_counts, out_status, gpf);
}
extern "C" int emus_sky_frame_reads(int digits, int max_iters) { return spx::host::sky_frame_reads(digits, max_iters); }
