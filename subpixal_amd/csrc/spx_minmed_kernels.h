// spx_minmed_kernels.h -- cosmic-ray rejection in two or three frames: the 'minmed' combination of the single-frame
// drizzles (step 2' of include/subpixal_hip.h) and the growth of a frame's cosmic-ray mask (step 7), modelled on
// drizzlepac's combine_type = 'minmed' / combine_grow and driz_cr_grow / driz_cr_ctegrow; drizzlepac is not in the
// reference tree, so parity with it is UNPINNED and the definition is this library's own (tests/minmed_statement.py
// restates it in numpy).  Three kernels for gfx950: drizzle_minmed_kernel<T>, minmed_grow_kernel and
// drizzle_cr_grow_kernel<T>.  Needs spx_crreject_kernels.h (and what that needs) first.
//
// Every decision is float64 with contraction off and made of + - * / and comparisons only (no sqrt), so that numpy
// reproduces it to the bit.  No kernel has an atomic, none reads a plane it also writes, and no result depends on the
// grid: a pixel's outputs are a function of the inputs alone.
#pragma once

#include <stdint.h>

namespace spx {

// ---------------------------------------------------------------------------------------------------------------
// Step 2', first pass.  drizzle_median_kernel's gather, LDS column and sort, unchanged (drz_frame_misses_tile,
// drz_frame_sums, float32 [nactive][256] of dynamic LDS), which also tracks the smallest valid value `lo` and the
// lowest row `kmin` that supplied it (rows are visited in ascending order and only a strictly smaller value takes
// over).  It takes 105 registers where the median takes 95, so it runs four waves per SIMD, not five; holding it
// to five (amdgpu_waves_per_eu) made the compiler spill 20 bytes per lane to scratch, and carrying the running
// minimum in the LDS column instead of a register saved one register: both were tried and dropped.
// tab : float64 [nframes][3] = (combine_rms, sky, gain) per table row; a gain that is not > 0: no Poisson term.
//   md   = step 2's median          lo = the minimum (0 where m = 0)          nmed = m
//   bits = hit_1 | hit_2 << 1,  hit_p = m >= 2 and t > 0 and t t > (n_p n_p) var,
//          t = (double)md - (double)lo,  var = r r + (g > 0 ? max((double)lo - sky, 0) / g : 0) of row kmin
// ---------------------------------------------------------------------------------------------------------------
template <typename T>
SPX_TKERNEL(256)
void drizzle_minmed_kernel(const DrizzleRow* __restrict__ rows, int nframes, int nactive, int kernel, int nlow,
                           int nhigh, const double* __restrict__ tab, double nsig1, double nsig2, int out_ny,
                           int out_nx, float* __restrict__ md, float* __restrict__ lo, uint8_t* __restrict__ bits,
                           uint8_t* __restrict__ nmed) {
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
        int m = 0, kmin = 0;
        float lov = 0.0f;
        for (int k = 0; k < nframes; ++k) {
            const DrizzleRow& r = rows[k];
            if (!r.active) continue;
            if (drz_frame_misses_tile(r, tcx, tcy, thx, thy)) continue;
            if (!inside) continue;
            double num = 0.0, den = 0.0;
            drz_frame_sums<T>(r, kernel, X, Y, num, den);
            if (den > 0.0 && m < nactive) {
                const float s = (float)(num / den);
                col[m * 256] = s;
                if (m == 0 || s < lov) {
                    lov = s;
                    kmin = k;
                }
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
        int first = 0, n = m;
        if (m - nlow - nhigh >= 1) {
            first = nlow;
            n = m - nlow - nhigh;
        }
        float v = 0.0f;
        if (n > 0) {
            const int mid = first + (n >> 1);
            v = (n & 1) ? col[mid * 256] : (float)(0.5 * ((double)col[(mid - 1) * 256] + (double)col[mid * 256]));
        }
        int hit = 0;
        if (m >= 2) {
            const double rr = tab[3 * kmin], sky = tab[3 * kmin + 1], g = tab[3 * kmin + 2];
            const double over = (double)lov - sky;
            double var = rr * rr;
            if (g > 0.0) var = var + (over > 0.0 ? over : 0.0) / g;
            const double t = (double)v - (double)lov;
            const double tt = t * t;
            if (t > 0.0) hit = (tt > (nsig1 * nsig1) * var ? 1 : 0) | (tt > (nsig2 * nsig2) * var ? 2 : 0);
        }
        const int64_t o = (int64_t)Y * out_nx + X;
        md[o] = v;
        lo[o] = lov;
        bits[o] = (uint8_t)hit;
        nmed[o] = (uint8_t)m;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Step 2', second pass: the neighbour rule.  A workgroup of 256 owns a 32 x 8 tile of output pixels and holds the
// decision bits of the tile and a halo of `grow` (0 .. 8) in dynamic LDS (kMmGrowLdsBytes: 48 x 24 bytes at most),
// 0 outside the grid.  seed = bit 0; use_min = seed or (bit 1 and a seed within Chebyshev distance grow).
//   med = use_min ? lo : md          minmed = 0 median, 1 minimum by the pixel's own test, 2 by the neighbour rule
// Only a pixel with bit 1 and without bit 0 looks at its neighbours.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kMmMaxGrow = 8;
constexpr size_t kMmGrowLdsBytes = (size_t)(kDrzTileW + 2 * kMmMaxGrow) * (kDrzTileH + 2 * kMmMaxGrow);

SPX_TKERNEL(256)
void minmed_grow_kernel(const float* __restrict__ md, const float* __restrict__ lo, const uint8_t* __restrict__ bits,
                        int grow, int out_ny, int out_nx, float* __restrict__ med, uint8_t* __restrict__ minmed) {
    SPX_DYN_LDS(s_bits);
    const int tid = rt::thread_id();
    const int W = kDrzTileW + 2 * grow, H = kDrzTileH + 2 * grow;
    const int64_t tiles_x = (out_nx + kDrzTileW - 1) / kDrzTileW, tiles_y = (out_ny + kDrzTileH - 1) / kDrzTileH;
    for (int64_t tile = rt::block_id(); tile < tiles_x * tiles_y; tile += rt::grid_size()) {
        const int X0 = (int)(tile % tiles_x) * kDrzTileW, Y0 = (int)(tile / tiles_x) * kDrzTileH;
        for (int p = tid; p < W * H; p += 256) {
            const int x = X0 - grow + p % W, y = Y0 - grow + p / W;
            const bool in = x >= 0 && x < out_nx && y >= 0 && y < out_ny;
            s_bits[p] = in ? bits[(int64_t)y * out_nx + x] : (uint8_t)0;
        }
        rt::block_sync();
        const int tx = tid & (kDrzTileW - 1), ty = tid / kDrzTileW;
        const int X = X0 + tx, Y = Y0 + ty;
        if (X < out_nx && Y < out_ny) {
            const int c = (ty + grow) * W + tx + grow;
            const int own = s_bits[c];
            int how = own & 1;
            if (!how && (own & 2)) {
                bool near = false;
                for (int dy = -grow; dy <= grow; ++dy)
                    for (int dx = -grow; dx <= grow; ++dx) near = near || (s_bits[c + dy * W + dx] & 1) != 0;
                if (near) how = 2;
            }
            const int64_t o = (int64_t)Y * out_nx + X;
            med[o] = how ? lo[o] : md[o];
            minmed[o] = (uint8_t)how;
        }
        rt::block_sync();                        // the next tile overwrites what this one reads
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Step 7: the growth of ONE frame's cosmic-ray mask.  seed = step 6's crmask.  A pixel that is not a seed is flagged
// iff it is testable in step 5's sense and a seed lies in the g x g block centred on it (g odd, 1 .. 9) or at
// (i, j - ctedir tau) for a tau = 1 .. c (c 0 .. 64, ctedir -1 | 0 | +1).  crmask = seed or flagged; clean is
// written ONLY at newly flagged pixels: (T)b with b of cr_blot_at, the comparison's own.
//
// A workgroup of 256 owns a 32 x 8 tile of the frame.  With h = (g - 1) / 2, U = max(h, ctedir > 0 ? c : 0) rows
// above and Dn = max(h, ctedir < 0 ? c : 0) rows below, dynamic LDS (kCrGrowLdsBytes) holds
//   S  the seeds of W = 32 + 2 h columns x R = 8 + U + Dn rows (0 outside the frame): each byte is loaded once
//   P  the exclusive prefix count of S down every column, R + 1 rows (one thread per column: a column scan), so
//      that "a seed in rows a .. b of column x" is P[b + 1][x] - P[a][x] != 0: the tail costs two LDS reads per
//      pixel whatever c is, and no global load
//   V  for the tile's 8 rows and all W columns: a seed within h rows; the block is the OR of g bytes of V
// Only a pixel with a seed in reach reads the frame, its weight, mask and rms, and evaluates the blot.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kCrGrowMaxHalf = 4, kCrGrowMaxCte = 64;
constexpr int kCrGrowW = kDrzTileW + 2 * kCrGrowMaxHalf;                           // 40
constexpr int kCrGrowR = kDrzTileH + kCrGrowMaxHalf + kCrGrowMaxCte;               // 76
constexpr size_t kCrGrowOffP = (size_t)kCrGrowW * kCrGrowR, kCrGrowOffV = kCrGrowOffP + (size_t)kCrGrowW * (kCrGrowR + 1);
constexpr size_t kCrGrowLdsBytes = kCrGrowOffV + (size_t)kCrGrowW * kDrzTileH;     // 3040 + 3080 + 320 = 6440

template <typename T>
SPX_TKERNEL(256)
void drizzle_cr_grow_kernel(const DrizzleRow* __restrict__ rows, int frame, const float* __restrict__ med,
                            const uint8_t* __restrict__ nmed, int out_ny, int out_nx, double rms_scalar,
                            const T* __restrict__ rms_map, const uint8_t* __restrict__ seed, int g, int c, int ctedir,
                            uint8_t* __restrict__ crmask, T* __restrict__ clean) {
    SPX_DYN_LDS(lds_raw);
    uint8_t* S = lds_raw;
    uint8_t* P = lds_raw + kCrGrowOffP;
    uint8_t* V = lds_raw + kCrGrowOffV;
    const int tid = rt::thread_id();
    const DrizzleRow& r = rows[frame];
    const int ny = r.ny, nx = r.nx;
    const T* __restrict__ Dd = static_cast<const T*>(r.data);
    const T* __restrict__ Ww = static_cast<const T*>(r.weight);
    const int h = (g - 1) / 2;
    if (ctedir == 0) c = 0;
    const int U = ctedir > 0 && c > h ? c : h, Dn = ctedir < 0 && c > h ? c : h;
    const int W = kDrzTileW + 2 * h, R = kDrzTileH + U + Dn;
    const int64_t tiles_x = (nx + kDrzTileW - 1) / kDrzTileW, tiles_y = (ny + kDrzTileH - 1) / kDrzTileH;
    for (int64_t tile = rt::block_id(); tile < tiles_x * tiles_y; tile += rt::grid_size()) {
        const int i0 = (int)(tile % tiles_x) * kDrzTileW, j0 = (int)(tile / tiles_x) * kDrzTileH;
        for (int p = tid; p < W * R; p += 256) {
            const int i = i0 - h + p % W, j = j0 - U + p / W;
            const bool in = i >= 0 && i < nx && j >= 0 && j < ny;
            S[p] = in && seed[(int64_t)j * nx + i] ? 1 : 0;
        }
        rt::block_sync();
        if (tid < W) {                               // the column scan
            int acc = 0;
            P[tid] = 0;
            for (int q = 0; q < R; ++q) {
                acc += S[q * W + tid];
                P[(q + 1) * W + tid] = (uint8_t)acc;
            }
        }
        rt::block_sync();
        for (int q = tid; q < kDrzTileH * W; q += 256) {
            const int row = q / W + U, x = q % W;
            V[q] = P[(row + h + 1) * W + x] != P[(row - h) * W + x] ? 1 : 0;
        }
        rt::block_sync();
        {
            const int tx = tid & (kDrzTileW - 1), ty = tid / kDrzTileW;
            const int i = i0 + tx, j = j0 + ty;
            if (i < nx && j < ny) {
                const int row = ty + U, x = tx + h;
                const int64_t q = (int64_t)j * nx + i;
                bool flag = S[row * W + x] != 0;
                if (!flag) {
                    bool reach = false;
                    for (int dx = 0; dx <= 2 * h; ++dx) reach = reach || V[ty * W + tx + dx] != 0;
                    if (ctedir > 0) reach = reach || P[row * W + x] != P[(row - c) * W + x];
                    if (ctedir < 0) reach = reach || P[(row + c + 1) * W + x] != P[(row + 1) * W + x];
                    if (reach) {
                        const T dv = Dd[q];
                        bool ok = (dv - dv == T(0)) && !(r.mask && r.mask[q]);
                        if (ok && Ww) {
                            const T wv = Ww[q];
                            ok = (wv - wv == T(0)) && wv > T(0);
                        }
                        if (ok) {
                            const double rms = rms_map ? (double)rms_map[q] : rms_scalar;
                            ok = (rms - rms == 0.0) && rms >= 0.0;
                        }
                        if (ok) {
                            float b;
                            if (cr_blot_at(r, med, nmed, out_ny, out_nx, i, j, b)) {
                                flag = true;
                                clean[q] = (T)b;
                            }
                        }
                    }
                }
                crmask[q] = flag ? 1 : 0;
            }
        }
        rt::block_sync();                        // the next tile overwrites what this one reads
    }
}

}  // namespace spx
