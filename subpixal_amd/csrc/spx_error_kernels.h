// spx_error_kernels.h -- per-source error measurements: what the reference's catalogue carries beside the
// positions (catalogs.py: fluxerr, fwhm -> pos_std -> weight) and align.find_linear_fit(use_weights=True)
// fits with.  One kernel, measure_errors_kernel, launched over labels 1..nlabels like measure_labels_kernel
// (spx_detect_kernels.h), whose table it reads: flux, x, y and peak come from that table's row, so the two
// kernels agree on them to the bit.  Needs spx_rt_hip.h (or the CPU harness) and spx_detect_kernels.h first.
//
// DEFINITIONS (tests/errors_statement.py states the same in numpy, float64)
//   A pixel p of label l inside boxes[l] is usable when v_p is finite, p is not masked and labels[p] == l
//   (the rule of measure_labels_kernel).  Over the usable pixels, in float64:
//     w_p  = v_p - bkg_p                        bkg_map in the frame's dtype when given, else bkg_scalar
//     s_p  = rms_p                              rms_map in the frame's dtype when given, else rms_scalar;
//                                               not finite or < 0: s_p = 0 and FLAG_NOISE is raised
//     v2_p = s_p * s_p + (w_p / gain  if gain > 0, gain finite and w_p > 0,  else 0)
//   fluxerr = sqrt(sum v2_p)                    SExtractor's FLUXERR_ISO, restated
//   ux = (xmin + dx) - x, uy = (ymin + dy) - y  (x, y the table's centre; dx, dy counted from the box's corner)
//   errx2 = sum(v2_p (ux ux)) / (flux flux), erry2 = sum(v2_p (uy uy)) / (flux flux),
//   errxy = sum(v2_p (ux uy)) / (flux flux)     the first-order variance of the flux-weighted centre
//                                               (d x / d I_p = (x_p - x) / flux); NaN unless flux > 0 and finite
//   nhalf = #{usable p : w_p >= 0.5 peak}       0 unless peak > 0
//   fwhm  = 2 sqrt(nhalf / pi)                  the diameter of the circle whose area is the half-maximum area;
//                                               NaN unless peak > 0
//   flags: kErrFlagHalfmax (32) when npix > 0 and nhalf == npix (the whole isophote lies above half maximum:
//          fwhm is a lower bound), kErrFlagNoise (64).
// out row l - 1 = (fluxerr, errx2, erry2, errxy, nhalf, fwhm).
// Every float sum is float64 in the FIXED order of measure_labels_kernel -- thread t takes box pixels t,
// t + 256, ... in turn, then a butterfly over the wave's lanes, then waves 0..3 in turn -- and contraction is off,
// so results are bit-identical from run to run and do not depend on the grid size.  There is one size class:
// every label takes one workgroup of 256.
#pragma once

namespace spx {

constexpr int kErrorCols = 6;                    // fluxerr errx2 erry2 errxy nhalf fwhm
constexpr int kErrFlagHalfmax = 32, kErrFlagNoise = 64;

template <typename T>
SPX_TKERNEL(256)
void measure_errors_kernel(const T* __restrict__ frame, const uint8_t* __restrict__ bad, double bkg_scalar,
                           const T* __restrict__ bkg_map, double rms_scalar, const T* __restrict__ rms_map,
                           double gain, const int32_t* __restrict__ labels, int fny, int fnx, int nlabels,
                           const int32_t* __restrict__ boxes, const double* __restrict__ table,
                           double* __restrict__ out, int32_t* __restrict__ out_flags) {
#pragma clang fp contract(off)
    SPX_DYN_LDS(lds_raw);
    double* red_d = reinterpret_cast<double*>(lds_raw);          // [4][4]
    int* red_i = reinterpret_cast<int*>(red_d + 16);             // [4][3]
    const int tid = rt::thread_id();
    const bool use_gain = gain > 0.0 && gain - gain == 0.0;
    for (int64_t lb = rt::block_id(); lb < nlabels; lb += rt::grid_size()) {
        const int l = (int)lb + 1;
        const int xmin = boxes[4 * l], ymin = boxes[4 * l + 1], xmax = boxes[4 * l + 2], ymax = boxes[4 * l + 3];
        const bool empty = xmax < xmin || ymax < ymin || xmin < 0 || ymin < 0 || xmax >= fnx || ymax >= fny;
        const int w = empty ? 1 : xmax - xmin + 1, h = empty ? 0 : ymax - ymin + 1;
        const int64_t n = (int64_t)w * h;
        const double* row = table + lb * kMeasureCols;
        const double flux = row[1], cx = row[2], cy = row[3], peak = row[10];
        const bool haspeak = peak > 0.0;
        const double half = 0.5 * peak;
        double S[4] = {0.0, 0.0, 0.0, 0.0};
        int npix = 0, nhalf = 0, noise = 0;
        for (int64_t i = tid; i < n; i += 256) {
            const int yy = (int)(i / w), xx = (int)(i - (int64_t)yy * w);
            const int64_t p = (int64_t)(ymin + yy) * fnx + xmin + xx;
            const T v = frame[p];
            if (!(v - v == T(0)) || (bad && bad[p])) continue;
            if (labels[p] != l) continue;
            const double wv = (double)v - (bkg_map ? (double)bkg_map[p] : bkg_scalar);
            double sg = rms_map ? (double)rms_map[p] : rms_scalar;
            if (!(sg - sg == 0.0) || sg < 0.0) {
                sg = 0.0;
                noise = 1;
            }
            const double v2 = sg * sg + (use_gain && wv > 0.0 ? wv / gain : 0.0);
            const double ux = (double)(xmin + xx) - cx, uy = (double)(ymin + yy) - cy;
            S[0] += v2;
            S[1] += v2 * (ux * ux);
            S[2] += v2 * (uy * uy);
            S[3] += v2 * (ux * uy);
            ++npix;
            if (haspeak && wv >= half) ++nhalf;
        }
        for (int m = 32; m >= 1; m >>= 1) {
            for (int k = 0; k < 4; ++k) S[k] += rt::shfl_xor(S[k], m);
            npix += rt::shfl_xor(npix, m);
            nhalf += rt::shfl_xor(nhalf, m);
            noise |= rt::shfl_xor(noise, m);
        }
        if ((tid & 63) == 0) {
            const int wv = tid >> 6;
            for (int k = 0; k < 4; ++k) red_d[wv * 4 + k] = S[k];
            red_i[wv * 3] = npix; red_i[wv * 3 + 1] = nhalf; red_i[wv * 3 + 2] = noise;
        }
        rt::block_sync();
        if (tid == 0) {
            for (int wv = 1; wv < 4; ++wv) {
                for (int k = 0; k < 4; ++k) S[k] += red_d[wv * 4 + k];
                npix += red_i[wv * 3];
                nhalf += red_i[wv * 3 + 1];
                noise |= red_i[wv * 3 + 2];
            }
            const double nan = __builtin_nan("");
            const bool pos = flux > 0.0 && flux - flux == 0.0;
            const double f2 = flux * flux;
            double* o = out + lb * kErrorCols;
            o[0] = sqrt(S[0]);
            o[1] = pos ? S[1] / f2 : nan;
            o[2] = pos ? S[2] / f2 : nan;
            o[3] = pos ? S[3] / f2 : nan;
            o[4] = (double)nhalf;
            o[5] = haspeak ? 2.0 * sqrt((double)nhalf / 3.14159265358979323846) : nan;
            out_flags[lb] = (npix > 0 && nhalf == npix ? kErrFlagHalfmax : 0) | (noise ? kErrFlagNoise : 0);
        }
        rt::block_sync();
    }
}
constexpr size_t kErrorLdsBytes = 16 * 8 + 12 * 4;

}  // namespace spx
