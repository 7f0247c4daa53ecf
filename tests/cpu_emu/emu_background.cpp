// TEST INFRASTRUCTURE ONLY: the background kernels (spx_background_kernels.h) on CPU threads (spx_rt_emu.h),
// launched in the order and with the LDS sizes of spx_capi.hip's background_mesh / background_maps, for
// tests/test_background_cpu.py.  Built on its own (one object, the Makefile's emu compiler and flags) so the main
// harness stays as it is.  Workgroups run one after another with real threads inside: this proves the kernels'
// logic, index arithmetic and barriers, not their speed.
#include "spx_rt_emu.h"

#include "spx_background_kernels.h"

using namespace spx;

namespace {
int64_t cap(int64_t blocks, int64_t most) { return blocks < 1 ? 1 : (blocks < most ? blocks : most); }

template <typename T>
int mesh(const T* frame, const uint8_t* bad, const int32_t* labels, int fny, int fnx, int bh, int bw, double kappa,
         int max_iters, double mgf, double* mb, double* mr, int32_t* ng, double* trace, int grid) {
    const int64_t ncells = (int64_t)((fny + bh - 1) / bh) * ((fnx + bw - 1) / bw);
    rt::launch(cap(ncells, grid), 256, [&] {
        bkg_cell_kernel<T>(frame, bad, labels, fny, fnx, bh, bw, kappa, max_iters, mgf, mb, mr, ng, trace);
    }, bkg_cell_lds_bytes(sizeof(T), bh, bw));
    return 0;
}

// `planes`: float64 [2][kBkgPlanes][ncy * ncx], the front of spx_background_maps_*'s workspace
template <typename T>
int maps(const double* mb, const double* mr, const int32_t* ng, int ncy, int ncx, int bh, int bw, int fs, int fny,
         int fnx, double nsigma, double* planes, T* bkg, T* rms, float* thr, int32_t* status, int grid) {
    const int64_t nc = (int64_t)ncy * ncx;
    int32_t ctl[64] = {0};
    *status = 0;
    double* fb = planes;
    double* fr = planes + (int64_t)kBkgPlanes * nc;
    rt::launch(cap((nc + 255) / 256, grid), 256, [&] { bkg_filter_kernel(mb, mr, ng, ncy, ncx, fs, fb, fr, ctl); }, 0);
    rt::launch(1, 256, [&] { bkg_global_kernel(mb, mr, ng, nc, fb, fr, ctl, status); }, kBkgGlobalLdsBytes);
    for (int phase = 0; phase < 2; ++phase) {
        const int64_t lines = 2 * (int64_t)(phase == 0 ? ncx + ncy : ncx);
        rt::launch(cap((lines + 255) / 256, grid), 256, [&] { bkg_spline_kernel(planes, ncy, ncx, phase); }, 0);
    }
    const int64_t groups = (int64_t)fny * ((fnx + 3) / 4);
    rt::launch(cap((groups + 255) / 256, grid), 256, [&] {
        bkg_expand_kernel<T>(planes, ncy, ncx, bh, bw, fny, fnx, nsigma, bkg, rms, thr);
    }, 0);
    return 0;
}
}  // namespace

extern "C" size_t emub_cell_lds_bytes(int elem, int bh, int bw) { return bkg_cell_lds_bytes((size_t)elem, bh, bw); }

extern "C" int emub_mesh_f32(const float* frame, const uint8_t* bad, const int32_t* labels, int fny, int fnx, int bh,
                             int bw, double kappa, int max_iters, double mgf, double* mb, double* mr, int32_t* ng,
                             double* trace, int grid) {
    return mesh<float>(frame, bad, labels, fny, fnx, bh, bw, kappa, max_iters, mgf, mb, mr, ng, trace, grid);
}
extern "C" int emub_mesh_f64(const double* frame, const uint8_t* bad, const int32_t* labels, int fny, int fnx, int bh,
                             int bw, double kappa, int max_iters, double mgf, double* mb, double* mr, int32_t* ng,
                             double* trace, int grid) {
    return mesh<double>(frame, bad, labels, fny, fnx, bh, bw, kappa, max_iters, mgf, mb, mr, ng, trace, grid);
}
extern "C" int emub_maps_f32(const double* mb, const double* mr, const int32_t* ng, int ncy, int ncx, int bh, int bw,
                             int fs, int fny, int fnx, double nsigma, double* planes, float* bkg, float* rms,
                             float* thr, int32_t* status, int grid) {
    return maps<float>(mb, mr, ng, ncy, ncx, bh, bw, fs, fny, fnx, nsigma, planes, bkg, rms, thr, status, grid);
}
extern "C" int emub_maps_f64(const double* mb, const double* mr, const int32_t* ng, int ncy, int ncx, int bh, int bw,
                             int fs, int fny, int fnx, double nsigma, double* planes, double* bkg, double* rms,
                             float* thr, int32_t* status, int grid) {
    return maps<double>(mb, mr, ng, ncy, ncx, bh, bw, fs, fny, fnx, nsigma, planes, bkg, rms, thr, status, grid);
}
