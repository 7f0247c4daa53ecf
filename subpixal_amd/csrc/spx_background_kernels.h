// spx_background_kernels.h -- sky background and noise maps on the device: the step in front of
// spx_detect_kernels.h that SExtractor calls the background mesh (the reference gets both maps from it,
// catalogs.py: SExImageCatalog).  frame -> (background, rms, threshold) without leaving the device.
//   bkg_cell_kernel<T>    one mesh cell per workgroup step: usable values -> LDS, sorted, sigma-clipped
//   bkg_filter_kernel     median filter of the two meshes over the good cells, one thread per cell
//   bkg_global_kernel     the median of all good cells for cells whose window holds none (one workgroup,
//                         returns at once when no cell asked for it)
//   bkg_spline_kernel     second-derivative planes of the natural cubic spline through the filtered meshes
//   bkg_expand_kernel<T>  bicubic evaluation at every pixel: background, rms and threshold maps
// Needs spx_rt_hip.h (or the CPU harness) first.  Plain C++ and vector stores only.
//
// DEFINITIONS (tests/background_statement.py states the same in numpy/scipy, float64; include/subpixal_hip.h
// carries them for callers)
//   mesh: cells of bh x bw pixels, ncy = ceil(fny / bh), ncx = ceil(fnx / bw); the last cell of an axis may be
//   partial.  usable(y,x) = finite(v) && !bad(y,x) && (no label image || labels(y,x) == 0).
//   Per cell, on the n usable values sorted ascending, range [lo, hi) = [0, n):
//     (1) med = median of sorted[lo:hi] (even count: (a + b) * 0.5 of the two middle values, in float64);
//     (2) if sorted[lo] == sorted[hi - 1] (all values equal): mean = that value, std = 0, stop.  Otherwise
//         mean = sum / m and std = sqrt(sum (v - mean)^2 / m), m = hi - lo, both sums float64 in a fixed order;
//     (3) stop if !(std > 0) or max_iters rounds are done;
//     (4) the new range is the part of [lo, hi) with med - kappa std <= v <= med + kappa std (two binary
//         searches); stop if it is the old range or would be empty (possible only for kappa < 1), else (1).
//   rms = std; bkg = mean if std == 0, 2.5 med - 1.5 mean if |mean - med| < 0.3 std, else med; ngood = n.
//   A cell is BAD when n < max(2, ceil(min_good_fraction * cell_pixels)), cell_pixels the true pixel count
//   of a partial cell: its bkg and rms are NaN (ngood still n).
//   Filter (fs in 1, 3, 5, 7; both meshes alike): every cell takes the median of the good cells (ngood >= 2,
//   bkg and rms not NaN) of the fs x fs window around it, truncated at the mesh border (even count: mean of
//   the two middle values); a window without a good cell: the median of all good cells of the mesh; a mesh
//   without a good cell raises bit 0 of the status word.
//   Expansion: tensor-product natural cubic spline through the filtered mesh, knots at the uniform cell
//   centres cy_j = j bh + (bh - 1) / 2, cx_i = i bw + (bw - 1) / 2 (a partial last cell too), pixel
//   coordinates clamped to [c_0, c_last]; one knot: constant, two: linear.  rms is clamped at 0 from below.
//   Everything up to the final rounding to the frame's dtype is float64.
//   thr = float32(double(bkg as stored) + nsigma * double(rms as stored)).
// Every sum is float64 in a FIXED order -- thread t takes elements lo + t, lo + t + 256, ... in turn, then 16
// threads add 16 partial sums each, then these 16 are added in turn -- and the sort's result does not depend on
// the order the values arrive in, so all results are bit-identical from run to run.
#pragma once

namespace spx {

typedef double bkg_f64x2 __attribute__((ext_vector_type(2)));

constexpr int kBkgMinBox = 8, kBkgMaxBox = 128;
constexpr int kBkgRedSlots = 256 + 16;             // float64 scratch of bkg_block_sum
constexpr int kBkgPlanes = 6;                      // per mesh: filtered z, z_yy, z_xx, z_xxyy, two solver scratch planes
constexpr size_t kBkgGlobalLdsBytes = (size_t)kBkgRedSlots * 8;

constexpr int bkg_pow2_at_least(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}
// most pixels of a cell: its values padded to a power of two fit 64 KiB of LDS
constexpr int bkg_max_cell_pixels(size_t elem) { return elem == 8 ? 8192 : 16384; }
// dynamic LDS of bkg_cell_kernel: reduction scratch [float64, kBkgRedSlots], the cell's values [T, power of two]
constexpr size_t bkg_cell_lds_bytes(size_t elem, int bh, int bw) {
    return (size_t)kBkgRedSlots * 8 + (size_t)bkg_pow2_at_least(bh * bw) * elem;
}

template <typename T> struct BkgVec;
template <> struct BkgVec<float> { typedef rt::f32x4 type; static constexpr int n = 4; };
template <> struct BkgVec<double> { typedef bkg_f64x2 type; static constexpr int n = 2; };

// sum of v over the 256 threads of the workgroup, the same value in every thread, in a fixed order.
// Two barriers; `red` may be reused by the next call at once (the slots a call writes before its first
// barrier are read only before its second one).
SPX_DEVICE double bkg_block_sum(double* red, double v) {
    const int tid = rt::thread_id();
    red[tid] = v;
    rt::block_sync_lds();
    if (tid < 16) {
        double s = 0.0;
        for (int k = 0; k < 16; ++k) s += red[16 * tid + k];
        red[256 + tid] = s;
    }
    rt::block_sync_lds();
    double s = 0.0;
    for (int k = 0; k < 16; ++k) s += red[256 + k];
    return s;
}

SPX_DEVICE void bkg_cell_finish(int n, int need, double med, double mean, double sd, double* bkg, double* rms,
                                int32_t* ngood) {
#pragma clang fp contract(off)
    const double nan = __builtin_nan("");
    double b = nan, r = nan;
    if (n >= need) {
        r = sd;
        if (sd == 0.0) b = mean;
        else if (__builtin_fabs(mean - med) < 0.3 * sd) b = 2.5 * med - 1.5 * mean;
        else b = med;
    }
    *bkg = b;
    *rms = r;
    *ngood = n;
}

// ---------------------------------------------------------------------------
// One 256-thread workgroup per cell.  The frame is read exactly once: every pixel of the cell goes to LDS,
// unusable ones as +inf, so that after the sort the n usable values come first and no compaction is needed.
// Rows are read with 16-byte loads when every row of the cell starts on a 16-byte boundary.
// The bitonic network runs over the next power of two of THIS cell's pixel count (a partial cell sorts less).
// LDS banks: a compare-exchange step of distance j >= 32 elements reads and writes consecutive addresses in
// consecutive lanes; the steps of distance 1..16 put the lanes of a half-wave on a stride of 2 elements
// (two-way conflicts for float32) -- 10 of the 78 steps of a 64 x 64 cell.
// trace: NULL, or float64 [ncells][5] = (lo, hi, med, mean, std) of each cell's last round (test harness only).
// ---------------------------------------------------------------------------
template <typename T>
SPX_TKERNEL(256)
void bkg_cell_kernel(const T* __restrict__ frame, const uint8_t* __restrict__ bad, const int32_t* __restrict__ labels,
                     int fny, int fnx, int bh, int bw, double kappa, int max_iters, double min_good_fraction,
                     double* __restrict__ mesh_bkg, double* __restrict__ mesh_rms, int32_t* __restrict__ mesh_ngood,
                     double* __restrict__ trace) {
    SPX_DYN_LDS(lds_raw);
    double* red = reinterpret_cast<double*>(lds_raw);
    T* val = reinterpret_cast<T*>(red + kBkgRedSlots);
    typedef typename BkgVec<T>::type VecT;
    constexpr int V = BkgVec<T>::n;
    const int tid = rt::thread_id();
    const int ncx = (fnx + bw - 1) / bw, ncy = (fny + bh - 1) / bh;
    const int64_t ncells = (int64_t)ncx * ncy;
    const bool rows16 = fnx % V == 0 && bw % V == 0 && reinterpret_cast<uintptr_t>(frame) % 16 == 0;
    const T inf = (T)__builtin_inf();
    for (int64_t cell = rt::block_id(); cell < ncells; cell += rt::grid_size()) {
        const int cyi = (int)(cell / ncx), cxi = (int)(cell - (int64_t)cyi * ncx);
        const int y0 = cyi * bh, x0 = cxi * bw;
        const int ch = fny - y0 < bh ? fny - y0 : bh, cw = fnx - x0 < bw ? fnx - x0 : bw;
        const int npx = ch * cw;
        int npad = 1;
        while (npad < npx) npad <<= 1;
        int cnt = 0;
        if (rows16 && cw % V == 0) {
            const int gpr = cw / V, ngroups = ch * gpr;
            for (int g = tid; g < ngroups; g += 256) {
                const int ly = g / gpr, lx = (g - ly * gpr) * V;
                const int64_t p = (int64_t)(y0 + ly) * fnx + x0 + lx;
                const VecT q = *reinterpret_cast<const VecT*>(frame + p);
                for (int k = 0; k < V; ++k) {
                    const T v = q[k];
                    const bool ok = (v - v == T(0)) && !(bad && bad[p + k]) && !(labels && labels[p + k] != 0);
                    val[ly * cw + lx + k] = ok ? v : inf;
                    cnt += ok ? 1 : 0;
                }
            }
        } else {
            for (int e = tid; e < npx; e += 256) {
                const int ly = e / cw, lx = e - ly * cw;
                const int64_t p = (int64_t)(y0 + ly) * fnx + x0 + lx;
                const T v = frame[p];
                const bool ok = (v - v == T(0)) && !(bad && bad[p]) && !(labels && labels[p] != 0);
                val[e] = ok ? v : inf;
                cnt += ok ? 1 : 0;
            }
        }
        for (int e = npx + tid; e < npad; e += 256) val[e] = inf;
        const int n = (int)bkg_block_sum(red, (double)cnt);      // its barriers also publish val
        // bitonic sort, ascending
        for (int k = 2; k <= npad; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < (npad >> 1); i += 256) {
                    const int a = ((i & ~(j - 1)) << 1) | (i & (j - 1)), b = a | j;
                    const bool up = (a & k) == 0;
                    const T va = val[a], vb = val[b];
                    if ((va > vb) == up) {
                        val[a] = vb;
                        val[b] = va;
                    }
                }
                rt::block_sync_lds();
            }
        }
        // sigma clipping: every thread carries the same lo, hi, med, mean, sd
        int lo = 0, hi = n;
        double med = 0.0, mean = 0.0, sd = 0.0;
        if (n > 0) {
            for (int it = 0;; ++it) {
                const int m = hi - lo, mid = lo + (m >> 1);
                med = (m & 1) ? (double)val[mid] : ((double)val[mid - 1] + (double)val[mid]) * 0.5;
                if (val[lo] == val[hi - 1]) {
                    mean = (double)val[lo];
                    sd = 0.0;
                    break;
                }
                double s = 0.0;
                for (int i = lo + tid; i < hi; i += 256) s += (double)val[i];
                mean = bkg_block_sum(red, s) / (double)m;
                double q = 0.0;
                for (int i = lo + tid; i < hi; i += 256) {
                    const double d = (double)val[i] - mean;
                    q += d * d;
                }
                sd = __builtin_sqrt(bkg_block_sum(red, q) / (double)m);
                if (!(sd > 0.0) || it >= max_iters) break;
                const double lower = med - kappa * sd, upper = med + kappa * sd;
                int a = lo, b = hi;                              // first index with v >= lower
                while (a < b) {
                    const int c = (a + b) >> 1;
                    if ((double)val[c] < lower) a = c + 1; else b = c;
                }
                const int nlo = a;
                b = hi;                                          // first index with v > upper
                while (a < b) {
                    const int c = (a + b) >> 1;
                    if ((double)val[c] <= upper) a = c + 1; else b = c;
                }
                const int nhi = a;
                if ((nlo == lo && nhi == hi) || nhi <= nlo) break;
                lo = nlo;
                hi = nhi;
            }
        }
        if (tid == 0) {
            const double want = __builtin_ceil(min_good_fraction * (double)npx);
            const int need = want > 2.0 ? (int)want : 2;
            bkg_cell_finish(n, need, med, mean, sd, mesh_bkg + cell, mesh_rms + cell, mesh_ngood + cell);
            if (trace) {                                         // the tests' view of the clipping: lo hi med mean std
                double* t = trace + 5 * cell;
                t[0] = (double)lo; t[1] = (double)hi; t[2] = med; t[3] = mean; t[4] = sd;
            }
        }
        rt::block_sync_lds();                                    // val is rewritten for the next cell
    }
}

SPX_DEVICE bool bkg_good(const double* mb, const double* mr, const int32_t* ng, int64_t c) {
    return ng[c] >= 2 && mb[c] == mb[c] && mr[c] == mr[c];
}

// median of v[0..n) (n <= 49), sorting in place
SPX_DEVICE double bkg_small_median(double* v, int n) {
    for (int i = 1; i < n; ++i) {
        const double x = v[i];
        int j = i - 1;
        while (j >= 0 && v[j] > x) {
            v[j + 1] = v[j];
            --j;
        }
        v[j + 1] = x;
    }
    return (n & 1) ? v[n >> 1] : (v[(n >> 1) - 1] + v[n >> 1]) * 0.5;
}

// ctl[0] is raised when a cell's window holds no good cell: that cell's outputs are NaN until bkg_global_kernel
SPX_TKERNEL(256)
void bkg_filter_kernel(const double* __restrict__ mesh_bkg, const double* __restrict__ mesh_rms,
                       const int32_t* __restrict__ mesh_ngood, int ncy, int ncx, int fs, double* __restrict__ filt_bkg,
                       double* __restrict__ filt_rms, int32_t* __restrict__ ctl) {
    const int64_t ncells = (int64_t)ncy * ncx;
    const int r = fs >> 1;
    for (int64_t c = rt::block_id() * 256 + rt::thread_id(); c < ncells; c += rt::grid_size() * 256) {
        const int j = (int)(c / ncx), i = (int)(c - (int64_t)j * ncx);
        double vb[49], vr[49];
        int n = 0;
        for (int jj = j - r; jj <= j + r; ++jj) {
            if (jj < 0 || jj >= ncy) continue;
            for (int ii = i - r; ii <= i + r; ++ii) {
                if (ii < 0 || ii >= ncx) continue;
                const int64_t q = (int64_t)jj * ncx + ii;
                if (!bkg_good(mesh_bkg, mesh_rms, mesh_ngood, q)) continue;
                vb[n] = mesh_bkg[q];
                vr[n] = mesh_rms[q];
                ++n;
            }
        }
        if (n == 0) {
            filt_bkg[c] = filt_rms[c] = __builtin_nan("");
            rt::atomic_max_i32(ctl, 1);
        } else {
            filt_bkg[c] = bkg_small_median(vb, n);
            filt_rms[c] = bkg_small_median(vr, n);
        }
    }
}

// the value of rank `rank` (0-based, ascending) among the good cells of `src`: a radix selection over the
// order-preserving integer image of the doubles, one bit per step, 64 counting passes
SPX_DEVICE double bkg_select(double* red, const double* src, const double* mb, const double* mr, const int32_t* ng,
                             int64_t ncells, int64_t rank) {
    unsigned long long prefix = 0;
    for (int bit = 63; bit >= 0; --bit) {
        const unsigned long long high = bit == 63 ? 0ull : (~0ull << (bit + 1));
        double cnt = 0.0;
        for (int64_t c = rt::thread_id(); c < ncells; c += 256) {
            if (!bkg_good(mb, mr, ng, c)) continue;
            const unsigned long long u = __builtin_bit_cast(unsigned long long, src[c]);
            const unsigned long long key = (u >> 63) ? ~u : (u | (1ull << 63));
            if ((key & high) == prefix && !((key >> bit) & 1)) cnt += 1.0;
        }
        const int64_t zeros = (int64_t)bkg_block_sum(red, cnt);
        if (rank >= zeros) {
            rank -= zeros;
            prefix |= 1ull << bit;
        }
    }
    const unsigned long long u = (prefix >> 63) ? (prefix & ~(1ull << 63)) : ~prefix;
    return __builtin_bit_cast(double, u);
}

// ONE workgroup.  Nothing to do unless bkg_filter_kernel raised ctl[0].
SPX_TKERNEL(256)
void bkg_global_kernel(const double* __restrict__ mesh_bkg, const double* __restrict__ mesh_rms,
                       const int32_t* __restrict__ mesh_ngood, int64_t ncells, double* __restrict__ filt_bkg,
                       double* __restrict__ filt_rms, const int32_t* __restrict__ ctl, int32_t* __restrict__ status) {
    SPX_DYN_LDS(lds_raw);
    double* red = reinterpret_cast<double*>(lds_raw);
    if (ctl[0] == 0) return;
    const int tid = rt::thread_id();
    double cnt = 0.0;
    for (int64_t c = tid; c < ncells; c += 256) cnt += bkg_good(mesh_bkg, mesh_rms, mesh_ngood, c) ? 1.0 : 0.0;
    const int64_t G = (int64_t)bkg_block_sum(red, cnt);
    if (G == 0) {
        if (tid == 0) status[0] = 1;
        return;
    }
    for (int m = 0; m < 2; ++m) {
        const double* src = m ? mesh_rms : mesh_bkg;
        double* dst = m ? filt_rms : filt_bkg;
        const double v1 = bkg_select(red, src, mesh_bkg, mesh_rms, mesh_ngood, ncells, (G - 1) >> 1);
        const double v2 = (G & 1) ? v1 : bkg_select(red, src, mesh_bkg, mesh_rms, mesh_ngood, ncells, G >> 1);
        const double gm = (G & 1) ? v1 : (v1 + v2) * 0.5;
        for (int64_t c = tid; c < ncells; c += 256)
            if (dst[c] != dst[c]) dst[c] = gm;
    }
}

// Natural cubic spline through z[0], z[stride], ... (n uniform knots): out = M h^2 / 6, M the second
// derivatives, i.e. out_0 = out_{n-1} = 0 and out_{i-1} + 4 out_i + out_{i+1} = z_{i-1} - 2 z_i + z_{i+1}.
// Thomas algorithm; `tmp` (same stride) holds the eliminated upper diagonal.
SPX_DEVICE void bkg_thomas(const double* z, int n, int64_t stride, double* out, double* tmp) {
#pragma clang fp contract(off)
    for (int i = 0; i < n; ++i) out[i * stride] = 0.0;
    if (n < 3) return;
    double cp = 0.0, dp = 0.0;
    for (int i = 1; i <= n - 2; ++i) {
        const double rhs = z[(i - 1) * stride] - 2.0 * z[i * stride] + z[(i + 1) * stride];
        const double den = 4.0 - cp;
        cp = 1.0 / den;
        dp = (rhs - dp) / den;
        tmp[i * stride] = cp;
        out[i * stride] = dp;
    }
    for (int i = n - 3; i >= 1; --i) out[i * stride] -= tmp[i * stride] * out[(i + 1) * stride];
}

// planes: [2 meshes][kBkgPlanes][ncy * ncx] float64 (plane 0 = filtered mesh, 1 = z_yy, 2 = z_xx, 3 = z_xxyy,
// 4 and 5 scratch).  phase 0: z_yy (one thread per mesh column) and z_xx (one per mesh row); phase 1: z_xxyy
// from z_xx (one per column).  One thread per line: the meshes are a few thousand nodes at most.
SPX_TKERNEL(256)
void bkg_spline_kernel(double* __restrict__ planes, int ncy, int ncx, int phase) {
    const int64_t nc = (int64_t)ncy * ncx;
    const int per = phase == 0 ? ncx + ncy : ncx;
    for (int64_t t = rt::block_id() * 256 + rt::thread_id(); t < 2 * (int64_t)per; t += rt::grid_size() * 256) {
        const int m = (int)(t / per), r = (int)(t - (int64_t)m * per);
        double* P = planes + (int64_t)m * kBkgPlanes * nc;
        if (phase == 0) {
            if (r < ncx) bkg_thomas(P + r, ncy, ncx, P + nc + r, P + 4 * nc + r);
            else bkg_thomas(P + (int64_t)(r - ncx) * ncx, ncx, 1, P + 2 * nc + (int64_t)(r - ncx) * ncx,
                            P + 5 * nc + (int64_t)(r - ncx) * ncx);
        } else {
            bkg_thomas(P + 2 * nc + r, ncy, ncx, P + 3 * nc + r, P + 4 * nc + r);
        }
    }
}

// where pixel coordinate p lies among n knots c_k = k * box + (box - 1) / 2: the interval and the weights of
// its two knots (A, B) and of their scaled second derivatives (A^3 - A, B^3 - B)
SPX_DEVICE void bkg_locate(int p, int n, int box, int& k0, int& k1, double* w) {
#pragma clang fp contract(off)
    if (n < 2) {
        k0 = k1 = 0;
        w[0] = 1.0; w[1] = 0.0; w[2] = 0.0; w[3] = 0.0;
        return;
    }
    const double c0 = 0.5 * (double)(box - 1), cl = c0 + (double)(n - 1) * (double)box;
    double pc = (double)p;
    pc = pc < c0 ? c0 : (pc > cl ? cl : pc);
    const double u = (pc - c0) / (double)box;
    int k = (int)u;
    if (k > n - 2) k = n - 2;
    const double B = u - (double)k, A = 1.0 - B;
    k0 = k;
    k1 = k + 1;
    w[0] = A; w[1] = B; w[2] = A * A * A - A; w[3] = B * B * B - B;
}

SPX_DEVICE void bkg_store4(float* p, const double* v) {
    *reinterpret_cast<rt::f32x4*>(p) = rt::f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
SPX_DEVICE void bkg_store4(double* p, const double* v) {
    bkg_f64x2* q = reinterpret_cast<bkg_f64x2*>(p);
    q[0] = bkg_f64x2{v[0], v[1]};
    q[1] = bkg_f64x2{v[2], v[3]};
}

// One thread per 4 consecutive pixels of a row, 16-byte stores when the rows allow it.  Along y the four
// planes are interpolated once per mesh column and kept while the pixels stay in the same x interval.
// Store-bound: the node planes are a few thousand doubles and stay in L2.
template <typename T>
SPX_TKERNEL(256)
void bkg_expand_kernel(const double* __restrict__ planes, int ncy, int ncx, int bh, int bw, int fny, int fnx,
                       double nsigma, T* __restrict__ bkg_out, T* __restrict__ rms_out, float* __restrict__ thr_out) {
    const int64_t nc = (int64_t)ncy * ncx;
    const int gpr = (fnx + 3) / 4;
    const int64_t total = (int64_t)fny * gpr;
    const bool vec = fnx % 4 == 0 && reinterpret_cast<uintptr_t>(bkg_out) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(rms_out) % 16 == 0 && reinterpret_cast<uintptr_t>(thr_out) % 16 == 0;
    for (int64_t g = rt::block_id() * 256 + rt::thread_id(); g < total; g += rt::grid_size() * 256) {
#pragma clang fp contract(off)
        const int y = (int)(g / gpr), x0 = (int)(g - (int64_t)y * gpr) * 4;
        int j0, j1;
        double wy[4];
        bkg_locate(y, ncy, bh, j0, j1, wy);
        int ilast = -1;
        double col[2][4];                 // per mesh: z(y, i0), z(y, i1), z_xx(y, i0), z_xx(y, i1)
        double ob[4], orms[4], oth[4];
        const int nk = fnx - x0 < 4 ? fnx - x0 : 4;
        for (int k = 0; k < nk; ++k) {
            int i0, i1;
            double wx[4];
            bkg_locate(x0 + k, ncx, bw, i0, i1, wx);
            if (i0 != ilast) {
                ilast = i0;
                for (int m = 0; m < 2; ++m) {
                    const double* Z = planes + (int64_t)m * kBkgPlanes * nc;
                    for (int s = 0; s < 2; ++s) {
                        const int64_t a = (int64_t)j0 * ncx + (s ? i1 : i0), b = (int64_t)j1 * ncx + (s ? i1 : i0);
                        col[m][s] = wy[0] * Z[a] + wy[1] * Z[b] + wy[2] * Z[nc + a] + wy[3] * Z[nc + b];
                        col[m][2 + s] = wy[0] * Z[2 * nc + a] + wy[1] * Z[2 * nc + b] + wy[2] * Z[3 * nc + a] +
                                        wy[3] * Z[3 * nc + b];
                    }
                }
            }
            const double vb = wx[0] * col[0][0] + wx[1] * col[0][1] + wx[2] * col[0][2] + wx[3] * col[0][3];
            double vr = wx[0] * col[1][0] + wx[1] * col[1][1] + wx[2] * col[1][2] + wx[3] * col[1][3];
            vr = vr < 0.0 ? 0.0 : vr;
            const double sb = (double)(T)vb, sr = (double)(T)vr;       // as stored
            ob[k] = vb;
            orms[k] = vr;
            oth[k] = sb + nsigma * sr;
        }
        const int64_t p = (int64_t)y * fnx + x0;
        if (vec) {
            if (bkg_out) bkg_store4(bkg_out + p, ob);
            if (rms_out) bkg_store4(rms_out + p, orms);
            if (thr_out) bkg_store4(thr_out + p, oth);
        } else {
            for (int k = 0; k < nk; ++k) {
                if (bkg_out) bkg_out[p + k] = (T)ob[k];
                if (rms_out) rms_out[p + k] = (T)orms[k];
                if (thr_out) thr_out[p + k] = (float)oth[k];
            }
        }
    }
}

}  // namespace spx
