// spx_crreject_kernels.h -- cosmic-ray rejection for the drizzle: the median of the single-frame drizzles, and per
// frame the blot of that median back onto the frame, its derivative, the two-threshold comparison and the cleaned
// frame (the steps the reference's Resample.execute runs between its two drizzles, resample.py:366-390; modelled on
// drizzlepac's createMedian / ablot / quickDeriv / drizCR; drizzlepac is not in the reference tree, so parity with
// it is UNPINNED and the definition is this library's own).  Two kernels: drizzle_median_kernel<T> and
// drizzle_cr_kernel<T>.  Needs spx_rt_hip.h (or the CPU harness), spx_aux_kernels.h (blot_resample) and
// spx_drizzle_kernels.h first.
//
// DEFINITION (include/subpixal_hip.h carries it in full; tests/crreject_statement.py states steps 2 .. 6 in numpy)
//   1. s_k(P) = (float)(num_k / wht_k): the drizzle's sums restricted to frame k; valid iff wht_k > 0.
//   2. med(P): the middle value of the m valid s_k sorted ascending, after the nlow lowest and nhigh highest are
//      dropped if that leaves one (else none are); even count: (float)(0.5 ((double)a + (double)b)); nmed = m.
//   3. b(i, j) = blot_resample(med, NY, NX, M_k(i, j)), defined iff M_k(i, j) lies in [0, NX-1] x [0, NY-1] and
//      every med pixel of the quintic's footprint [ix-2, ix+3] x [iy-2, iy+3], clipped to the grid, has nmed > 0.
//   4. D(i, j) = max |b(i, j) - b(n)| over the four neighbours n whose b is defined, 0 if none is.
//   5. fail_p = testable and |d - b| > scale_p D + snr_p sqrt(rms^2 + max(b - sky, 0) / gain), p = 1, 2, float64.
//   6. crmask = fail_2 and (a pixel of the 3 x 3 block has fail_1); clean = crmask ? (T)b : d.
#pragma once

#include <math.h>
#include <stdint.h>

namespace spx {

// ---------------------------------------------------------------------------------------------------------------
// The median.  The gather of drizzle_kernel (same tile, same frame-against-tile skip, same window and overlap:
// drz_frame_misses_tile and drz_frame_sums are the drizzle's own), with the sums started from 0 for every frame.
// One thread owns one output pixel and the column [slot][tid] of a dynamic-LDS array float32 [nactive][256]: lane
// t of a wave reads and writes word slot * 256 + t, so the 64 lanes hit 64 consecutive words and no bank twice.
// Nothing is shared between threads: no barrier, no atomic, the result does not depend on the grid.
// `nactive` sizes the column: a valid value beyond it would be dropped (the host passes the count of active rows).
// ---------------------------------------------------------------------------------------------------------------
constexpr size_t drizzle_median_lds_bytes(int nactive) { return (size_t)nactive * 256 * sizeof(float); }

template <typename T>
SPX_TKERNEL(256)
void drizzle_median_kernel(const DrizzleRow* __restrict__ rows, int nframes, int nactive, int kernel, int nlow,
                           int nhigh, int out_ny, int out_nx, float* __restrict__ med, uint8_t* __restrict__ nmed) {
#pragma clang fp contract(off)
    SPX_DYN_LDS(lds_raw);
    const int tid = rt::thread_id();
    float* col = reinterpret_cast<float*>(lds_raw) + tid;
    const int64_t tiles_x = (out_nx + kDrzTileW - 1) / kDrzTileW, tiles_y = (out_ny + kDrzTileH - 1) / kDrzTileH;
    for (int64_t tile = rt::block_id(); tile < tiles_x * tiles_y; tile += rt::grid_size()) {
        const int X0 = (int)(tile % tiles_x) * kDrzTileW, Y0 = (int)(tile / tiles_x) * kDrzTileH;
        const int X = X0 + (tid & (kDrzTileW - 1)), Y = Y0 + tid / kDrzTileW;
        const bool inside = X < out_nx && Y < out_ny;
        const double tcx = (double)X0 + 0.5 * (kDrzTileW - 1), tcy = (double)Y0 + 0.5 * (kDrzTileH - 1);
        const double thx = 0.5 * (kDrzTileW - 1), thy = 0.5 * (kDrzTileH - 1);
        int m = 0;
        for (int k = 0; k < nframes; ++k) {
            const DrizzleRow& r = rows[k];
            if (!r.active) continue;
            if (drz_frame_misses_tile(r, tcx, tcy, thx, thy)) continue;
            if (!inside) continue;
            double num = 0.0, den = 0.0;
            drz_frame_sums<T>(r, kernel, X, Y, num, den);
            if (den > 0.0 && m < nactive) {
                col[m * 256] = (float)(num / den);
                ++m;
            }
        }
        if (!inside) continue;
        for (int q = 1; q < m; ++q) {                 // insertion sort of the thread's own column, ascending
            const float v = col[q * 256];
            int p = q - 1;
            while (p >= 0 && col[p * 256] > v) {
                col[(p + 1) * 256] = col[p * 256];
                --p;
            }
            col[(p + 1) * 256] = v;
        }
        int lo = 0, n = m;
        if (m - nlow - nhigh >= 1) {
            lo = nlow;
            n = m - nlow - nhigh;
        }
        float v = 0.0f;
        if (n > 0) {
            const int mid = lo + (n >> 1);
            v = (n & 1) ? col[mid * 256] : (float)(0.5 * ((double)col[(mid - 1) * 256] + (double)col[mid * 256]));
        }
        const int64_t o = (int64_t)Y * out_nx + X;
        med[o] = v;
        nmed[o] = (uint8_t)m;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Blot, derivative, comparison, mask and cleaned frame of ONE frame.  A workgroup of 256 owns a 32 x 8 tile of
// INPUT pixels.  Dynamic LDS (kCrLdsBytes):
//   phase A  b and its defined-flag on the tile + a halo of 2 (36 x 12 = 432 positions, strided over the threads);
//            d, rms and testability on the tile + a halo of 1 (34 x 10 = 340)
//   phase B  D and fail_1 on the tile + a halo of 1
//   phase C  fail_2 of the thread's own pixel, the 3 x 3 block of fail_1, crmask and clean
// Positions outside the frame have a b (the map is defined there) and are never testable.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kCrBW = kDrzTileW + 4, kCrBH = kDrzTileH + 4, kCrBN = kCrBW * kCrBH;        // 36 x 12 = 432
constexpr int kCrHW = kDrzTileW + 2, kCrHH = kDrzTileH + 2, kCrHN = kCrHW * kCrHH;        // 34 x 10 = 340
constexpr int kCrMinOut = 6;                      // the quintic's edge continuation needs a 6 x 6 median at least
// double d[340], rms[340] | float b[432], D[340] | uint8 bdef[432], testable[340], fail1[340]
constexpr size_t kCrOffB = (size_t)2 * kCrHN * 8, kCrOffD = kCrOffB + (size_t)kCrBN * 4;
constexpr size_t kCrOffFlags = kCrOffD + (size_t)kCrHN * 4;
constexpr size_t kCrLdsBytes = kCrOffFlags + kCrBN + 2 * kCrHN;

struct CrParams {
    double rms_scalar, sky, gain;                 // gain: 0 where the caller's is not finite or not > 0 (no Poisson term)
    double snr1, snr2, scale1, scale2;
};

namespace host {
inline CrParams cr_params(double rms_scalar, double sky, double gain, double snr1, double snr2, double scale1,
                          double scale2) {
    CrParams c;
    c.rms_scalar = rms_scalar;
    c.sky = sky;
    c.gain = (gain - gain == 0.0 && gain > 0.0) ? gain : 0.0;
    c.snr1 = snr1;
    c.snr2 = snr2;
    c.scale1 = scale1;
    c.scale2 = scale2;
    return c;
}
}  // namespace host

// t > scale D + snr sqrt(rms^2 + max(b - sky, 0) / gain), float64
SPX_DEVICE bool cr_fails(double d, float b, float D, double rms, const CrParams& c, double scale, double snr) {
#pragma clang fp contract(off)
    const double t = fabs(d - (double)b);
    const double over = (double)b - c.sky;
    double var = rms * rms;
    if (c.gain > 0.0) var = var + (over > 0.0 ? over : 0.0) / c.gain;
    return t > scale * (double)D + snr * sqrt(var);
}

// step 3 at ONE position (i, j) of row r's frame (inside it or not): b and whether it is defined; b = 0 where it is
// not.  drizzle_cr_kernel's phase A and the grow pass of spx_minmed_kernels.h share it, so that the b a grown pixel
// gets is the b the comparison saw: the same operations in the same order.
SPX_DEVICE bool cr_blot_at(const DrizzleRow& r, const float* __restrict__ med, const uint8_t* __restrict__ nmed,
                           int out_ny, int out_nx, int i, int j, float& b) {
#pragma clang fp contract(off)
    const double X = (r.a[0] * (double)i + r.a[1] * (double)j) + r.a[2];
    const double Y = (r.a[3] * (double)i + r.a[4] * (double)j) + r.a[5];
    bool def = X >= 0.0 && X <= (double)(out_nx - 1) && Y >= 0.0 && Y <= (double)(out_ny - 1);
    b = 0.0f;
    if (def) {
        const int ix = (int)X, iy = (int)Y;
        const int xa = ix - 2 < 0 ? 0 : ix - 2, xb = ix + 3 > out_nx - 1 ? out_nx - 1 : ix + 3;
        const int ya = iy - 2 < 0 ? 0 : iy - 2, yb = iy + 3 > out_ny - 1 ? out_ny - 1 : iy + 3;
        for (int y = ya; y <= yb; ++y)
            for (int x = xa; x <= xb; ++x) def = def && nmed[(int64_t)y * out_nx + x] != 0;
        if (def) b = blot_resample(med, out_ny, out_nx, X, Y);
    }
    return def;
}

template <typename T>
SPX_TKERNEL(256)
void drizzle_cr_kernel(const DrizzleRow* __restrict__ rows, int frame, const float* __restrict__ med,
                       const uint8_t* __restrict__ nmed, int out_ny, int out_nx, const T* __restrict__ rms_map,
                       CrParams c, uint8_t* __restrict__ crmask, T* __restrict__ clean) {
#pragma clang fp contract(off)
    SPX_DYN_LDS(lds_raw);
    double* s_d = reinterpret_cast<double*>(lds_raw);
    double* s_rms = s_d + kCrHN;
    float* s_b = reinterpret_cast<float*>(lds_raw + kCrOffB);
    float* s_D = reinterpret_cast<float*>(lds_raw + kCrOffD);
    uint8_t* s_bdef = lds_raw + kCrOffFlags;
    uint8_t* s_test = s_bdef + kCrBN;
    uint8_t* s_fail1 = s_test + kCrHN;
    const int tid = rt::thread_id();
    const DrizzleRow& r = rows[frame];
    const int ny = r.ny, nx = r.nx;
    const T* __restrict__ Dd = static_cast<const T*>(r.data);
    const T* __restrict__ Ww = static_cast<const T*>(r.weight);
    const int64_t tiles_x = (nx + kDrzTileW - 1) / kDrzTileW, tiles_y = (ny + kDrzTileH - 1) / kDrzTileH;
    for (int64_t tile = rt::block_id(); tile < tiles_x * tiles_y; tile += rt::grid_size()) {
        const int i0 = (int)(tile % tiles_x) * kDrzTileW, j0 = (int)(tile / tiles_x) * kDrzTileH;
        // phase A: the blot
        for (int p = tid; p < kCrBN; p += 256) {
            float b;
            const bool def = cr_blot_at(r, med, nmed, out_ny, out_nx, i0 - 2 + p % kCrBW, j0 - 2 + p / kCrBW, b);
            s_b[p] = b;
            s_bdef[p] = def ? 1 : 0;
        }
        // phase A: the frame
        for (int h = tid; h < kCrHN; h += 256) {
            const int i = i0 - 1 + h % kCrHW, j = j0 - 1 + h / kCrHW;
            double d = 0.0, rms = 0.0;
            bool ok = i >= 0 && i < nx && j >= 0 && j < ny;
            if (ok) {
                const int64_t q = (int64_t)j * nx + i;
                const T dv = Dd[q];
                d = (double)dv;
                ok = (dv - dv == T(0)) && !(r.mask && r.mask[q]);
                if (ok && Ww) {
                    const T wv = Ww[q];
                    ok = (wv - wv == T(0)) && wv > T(0);
                }
                if (ok) {
                    rms = rms_map ? (double)rms_map[q] : c.rms_scalar;
                    ok = (rms - rms == 0.0) && rms >= 0.0;
                }
            }
            s_d[h] = d;
            s_rms[h] = rms;
            s_test[h] = ok ? 1 : 0;                  // b's flag joins in phase B, after the barrier
        }
        rt::block_sync();
        // phase B: the derivative and the first test
        for (int h = tid; h < kCrHN; h += 256) {
            const int p = (h / kCrHW + 1) * kCrBW + h % kCrHW + 1;
            const float b = s_b[p];
            float D = 0.0f;
            const int nb[4] = {p - 1, p + 1, p - kCrBW, p + kCrBW};
            for (int q = 0; q < 4; ++q)
                if (s_bdef[nb[q]]) {
                    const float e = fabsf(b - s_b[nb[q]]);
                    D = e > D ? e : D;
                }
            const bool ok = s_test[h] && s_bdef[p];
            s_D[h] = D;
            s_test[h] = ok ? 1 : 0;
            s_fail1[h] = ok && cr_fails(s_d[h], b, D, s_rms[h], c, c.scale1, c.snr1) ? 1 : 0;
        }
        rt::block_sync();
        // phase C: the second test, the neighbour rule, the outputs
        {
            const int tx = tid & (kDrzTileW - 1), ty = tid / kDrzTileW;
            const int i = i0 + tx, j = j0 + ty;
            if (i < nx && j < ny) {
                const int h = (ty + 1) * kCrHW + tx + 1, p = (ty + 2) * kCrBW + tx + 2;
                bool flag = false;
                if (s_test[h] && cr_fails(s_d[h], s_b[p], s_D[h], s_rms[h], c, c.scale2, c.snr2)) {
                    for (int dy = -1; dy <= 1; ++dy)
                        for (int dx = -1; dx <= 1; ++dx) flag = flag || s_fail1[h + dy * kCrHW + dx] != 0;
                }
                const int64_t q = (int64_t)j * nx + i;
                crmask[q] = flag ? 1 : 0;
                clean[q] = flag ? (T)s_b[p] : Dd[q];
            }
        }
        rt::block_sync();                        // the next tile overwrites what phase C reads
    }
}

}  // namespace spx
