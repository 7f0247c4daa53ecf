// TEST INFRASTRUCTURE ONLY: the error-measurement kernel (spx_error_kernels.h) on CPU threads (spx_rt_emu.h),
// launched with the LDS size of spx_capi.hip's measure_errors, for tests/test_errors_cpu.py.  It sits on top of
// emu_detect.cpp, whose emud_label_bboxes / emud_measure_* give the boxes and the measure table the kernel reads,
// as the library's own kernels do.  Built on its own (one object, the Makefile's emu compiler and flags).
// As there, the workgroups of a launch run ONE AFTER ANOTHER with real threads inside a workgroup.
#include "emu_detect.cpp"

#include "spx_error_kernels.h"

namespace {
template <typename T>
int errors(const T* frame, const uint8_t* bad, double bkg, const T* bkg_map, double rms, const T* rms_map, double gain,
           const int32_t* labels, int fny, int fnx, int nlabels, const int32_t* boxes, const double* table,
           double* out, int32_t* eflags, int grid) {
    if (nlabels == 0) return 0;
    rt::launch(cap(nlabels, grid), 256, [&] {
        measure_errors_kernel<T>(frame, bad, bkg, bkg_map, rms, rms_map, gain, labels, fny, fnx, nlabels, boxes, table,
                                 out, eflags);
    }, kErrorLdsBytes);
    return 0;
}
}  // namespace

extern "C" int emue_errors_f32(const float* frame, const uint8_t* bad, double bkg, const float* bkg_map, double rms,
                               const float* rms_map, double gain, const int32_t* labels, int fny, int fnx,
                               int nlabels, const int32_t* boxes, const double* table, double* out, int32_t* eflags,
                               int grid) {
    return errors<float>(frame, bad, bkg, bkg_map, rms, rms_map, gain, labels, fny, fnx, nlabels, boxes, table, out,
                         eflags, grid);
}
extern "C" int emue_errors_f64(const double* frame, const uint8_t* bad, double bkg, const double* bkg_map, double rms,
                               const double* rms_map, double gain, const int32_t* labels, int fny, int fnx,
                               int nlabels, const int32_t* boxes, const double* table, double* out, int32_t* eflags,
                               int grid) {
    return errors<double>(frame, bad, bkg, bkg_map, rms, rms_map, gain, labels, fny, fnx, nlabels, boxes, table, out,
                          eflags, grid);
}
