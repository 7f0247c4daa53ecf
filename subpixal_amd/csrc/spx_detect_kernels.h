// spx_detect_kernels.h -- source finding on the device: what the reference leaves to SExtractor
// (catalogs.py: ImageCatalog / SExImageCatalog) and the catalog path of align.find_linear_fit needs
// before it can start: a segmentation image and one position per segment.
//   detect_tile_kernel      detection mask + connected-component merge of one 64x32 tile in LDS
//   detect_border_kernel    merge across tile borders in global memory
//   detect_compress_kernel  every pixel -> the root of its component, pixels counted per root
//   detect_flag_count_kernel / detect_scan_blocks_kernel / detect_assign_kernel / detect_relabel_kernel
//                           minimum area, numbering 1..L in raster order of the first pixel, final label image
//   measure_labels_kernel   isophotal measurements, one workgroup per label over the label's bounding box
// Needs spx_rt_hip.h (or the CPU harness) first.  Plain C++ and vector atomics only.
//
// DEFINITIONS (the tests state the same in numpy/scipy, float64)
//   detected(y,x) = finite(v) && !bad(y,x) && f(y,x) > thr(y,x)         strict >, NaN thresholds detect nothing
//   f = v without a filter; with a filter k [fky][fkx] (odd sides <= 7, centre at (fky/2, fkx/2))
//       f(y,x) = sum_{j,i} k[j][i] * v'(y + j - fky/2, x + i - fkx/2)    (a correlation, not a convolution)
//     where v' = v, or 0 for pixels outside the frame, masked or not finite.  The weights are used AS GIVEN:
//     neither the kernel nor the Python wrapper normalises them, and they are NOT renormalised where
//     pixels drop out.  The sum runs row-major over the kernel (j outer, i inner) as one fused multiply-add
//     chain acc = fma(k[j][i], v', acc) from acc = 0 in the frame's dtype.
//   thr = thr_scalar, or thr_map(y,x) (float32, converted exactly to the frame's dtype) when a map is given.
//   Components: 8-connectivity (or 4); the root of a component is its first pixel in raster order (the
//   smallest linear index), whatever the scheduling: unions only ever lower a parent (atomic min).
//
// LABEL ENCODING while merging: L[p] = (linear index of p's parent) + 1, 0 = background; a root points at
// itself.  Parents only decrease, so every chain is strictly decreasing and ends; a link that does not
// decrease (which no schedule can produce) or a chain above kDetMaxChain hops raises the status word and the
// call reports it (out_nlabels = -1) instead of spinning.
#pragma once

namespace spx {

constexpr int kDetTW = 64, kDetTH = 32;          // tile of the local merge: 2048 labels = 8 KiB of LDS
constexpr int kDetMaxFilter = 7;
constexpr int kDetMaxChain = 1 << 24;
constexpr int kDetChunk = 1024;                  // pixels per workgroup step of the numbering kernels
constexpr int kMeasureCols = 13;                 // npix flux x y x2 y2 xy a b theta peak xpeak ypeak

// dynamic LDS of detect_tile_kernel: frame tile with halo [T], filter [T, 56 slots], labels [int32]
constexpr int det_tile_elems(int fky, int fkx) {
    return ((kDetTH + fky - 1) * (kDetTW + fkx - 1) + 1) / 2 * 2;
}
constexpr size_t det_tile_lds_bytes(size_t elem, int fky, int fkx) {
    return (size_t)(det_tile_elems(fky, fkx) + 56) * elem + (size_t)kDetTW * kDetTH * 4;
}

SPX_DEVICE float det_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
SPX_DEVICE double det_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// the filter sum of the DEFINITIONS at one pixel; v(j, i) = v' at row j, column i of the kernel's footprint
template <typename T, typename V>
SPX_DEVICE T det_filter_chain(const T* fk, int fky, int fkx, V v) {
    T f = T(0);
    for (int j = 0; j < fky; ++j)
        for (int k = 0; k < fkx; ++k) f = det_fma(fk[j * fkx + k], v(j, k), f);
    return f;
}

SPX_DEVICE int det_find(const int32_t* L, int p, int& err) {
    for (int it = 0; it < kDetMaxChain; ++it) {
        const int q = rt::atomic_load_i32(L + p) - 1;
        if (q == p) return p;
        if (q < 0 || q > p) break;
        p = q;
    }
    err = 1;
    return p;
}

// joins the components of pixels a and b: the larger root is linked below the smaller one
SPX_DEVICE void det_union(int32_t* L, int a, int b, int& err) {
    for (int it = 0; it < kDetMaxChain; ++it) {
        a = det_find(L, a, err);
        b = det_find(L, b, err);
        if (err || a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = rt::atomic_min_ret_i32(L + a, b + 1) - 1;
        if (old == a) return;                    // a was still a root: linked
        a = old;                                 // a was linked elsewhere meanwhile: that set and b's must meet too
    }
    err = 1;
}

// ---------------------------------------------------------------------------
// (a) + local part of (b): one tile per workgroup step.  Writes L (root of the pixel WITHIN ITS TILE, as a
// global linear index + 1) and clears cnt for every pixel of the frame.
// ---------------------------------------------------------------------------
template <typename T>
SPX_TKERNEL(256)
void detect_tile_kernel(const T* __restrict__ frame, const uint8_t* __restrict__ bad, T thr_scalar,
                        const float* __restrict__ thr_map, const T* __restrict__ filt, int fky, int fkx, int fny,
                        int fnx, int conn, int32_t* __restrict__ L, int32_t* __restrict__ cnt,
                        int32_t* __restrict__ status) {
    SPX_DYN_LDS(lds_raw);
    const int tid = rt::thread_id();
    const int hy = fky / 2, hx = fkx / 2;
    const int frw = kDetTW + fkx - 1, frh = kDetTH + fky - 1;
    T* fr = reinterpret_cast<T*>(lds_raw);
    T* fk = fr + det_tile_elems(fky, fkx);
    int32_t* lab = reinterpret_cast<int32_t*>(fk + 56);
    const int ntx = (fnx + kDetTW - 1) / kDetTW, nty = (fny + kDetTH - 1) / kDetTH;
    const int64_t ntiles = (int64_t)ntx * nty;
    int err = 0;
    for (int64_t tile = rt::block_id(); tile < ntiles; tile += rt::grid_size()) {
        const int ty0 = (int)(tile / ntx) * kDetTH, tx0 = (int)(tile % ntx) * kDetTW;
        // stage: v' with halo; lab = 1 where the pixel itself may be detected
        for (int e = tid; e < frh * frw; e += 256) {
            const int ly = e / frw, lx = e - ly * frw;
            const int gy = ty0 + ly - hy, gx = tx0 + lx - hx;
            T v = T(0);
            bool ok = false;
            if (gy >= 0 && gy < fny && gx >= 0 && gx < fnx) {
                const int64_t g = (int64_t)gy * fnx + gx;
                v = frame[g];
                ok = (v - v == T(0)) && !(bad && bad[g]);
                if (!ok) v = T(0);
            }
            fr[e] = v;
            const int iy = ly - hy, ix = lx - hx;
            if (iy >= 0 && iy < kDetTH && ix >= 0 && ix < kDetTW) lab[iy * kDetTW + ix] = ok ? 1 : 0;
        }
        if (filt && tid < fky * fkx) fk[tid] = filt[tid];
        rt::block_sync();
        const int lx = tid & (kDetTW - 1);
        for (int ly = tid >> 6; ly < kDetTH; ly += 4) {
            const int i = ly * kDetTW + lx;
            if (!lab[i]) continue;
            T f;
            if (filt) {
                f = det_filter_chain<T>(fk, fky, fkx, [&](int j, int k) { return fr[(ly + j) * frw + lx + k]; });
            } else {
                f = fr[(ly + hy) * frw + lx + hx];
            }
            const T thr = thr_map ? (T)thr_map[(int64_t)(ty0 + ly) * fnx + tx0 + lx] : thr_scalar;
            lab[i] = f > thr ? i + 1 : 0;
        }
        rt::block_sync();
        // local merge with the neighbours that come earlier in raster order
        for (int ly = tid >> 6; ly < kDetTH; ly += 4) {
            const int i = ly * kDetTW + lx;
            if (!rt::atomic_load_i32(lab + i)) continue;
            if (lx > 0 && rt::atomic_load_i32(lab + i - 1)) det_union(lab, i, i - 1, err);
            if (ly > 0) {
                if (rt::atomic_load_i32(lab + i - kDetTW)) det_union(lab, i, i - kDetTW, err);
                if (conn == 8) {
                    if (lx > 0 && rt::atomic_load_i32(lab + i - kDetTW - 1)) det_union(lab, i, i - kDetTW - 1, err);
                    if (lx < kDetTW - 1 && rt::atomic_load_i32(lab + i - kDetTW + 1))
                        det_union(lab, i, i - kDetTW + 1, err);
                }
            }
        }
        rt::block_sync();
        for (int ly = tid >> 6; ly < kDetTH; ly += 4) {
            const int gy = ty0 + ly, gx = tx0 + lx;
            if (gy >= fny || gx >= fnx) continue;
            const int i = ly * kDetTW + lx;
            int32_t out = 0;
            if (lab[i]) {
                const int r = det_find(lab, i, err);
                out = (ty0 + r / kDetTW) * fnx + tx0 + (r & (kDetTW - 1)) + 1;
            }
            const int64_t g = (int64_t)gy * fnx + gx;
            L[g] = out;
            cnt[g] = 0;
        }
        rt::block_sync();
    }
    if (err) rt::atomic_max_i32(status, 1);
}

// ---------------------------------------------------------------------------
// (b) across tiles.  Work items: the pixels of every tile's first row, first column and last column, i.e.
// all pixels with an earlier-in-raster-order neighbour in another tile.
// ---------------------------------------------------------------------------
SPX_TKERNEL(256)
void detect_border_kernel(int32_t* __restrict__ L, int fny, int fnx, int conn, int32_t* __restrict__ status) {
    const int ntx = (fnx + kDetTW - 1) / kDetTW, nty = (fny + kDetTH - 1) / kDetTH;
    const int64_t nrow = (int64_t)(nty - 1) * fnx, ncol = (int64_t)(ntx - 1) * fny;
    const int64_t total = nrow + 2 * ncol;
    const int64_t step = rt::grid_size() * 256;
    int err = 0;
    for (int64_t i = rt::block_id() * 256 + rt::thread_id(); i < total; i += step) {
        int y, x;
        if (i < nrow) {
            y = (int)(i / fnx + 1) * kDetTH;
            x = (int)(i % fnx);
        } else {
            const int64_t k = i - nrow;
            const int right = k >= ncol;
            const int64_t kk = right ? k - ncol : k;
            x = (int)(kk / fny + 1) * kDetTW - right;
            y = (int)(kk % fny);
        }
        const int p = y * fnx + x;
        if (!rt::atomic_load_i32(L + p)) continue;
        const int nnb = conn == 8 ? 4 : 2;
        for (int n = 0; n < nnb; ++n) {
            // 4-connectivity: W, N; 8-connectivity: W, N, NW, NE
            const int dy = n == 0 ? 0 : -1, dx = n == 0 ? -1 : (n == 1 ? 0 : (n == 2 ? -1 : 1));
            const int qy = y + dy, qx = x + dx;
            if (qy < 0 || qx < 0 || qx >= fnx) continue;
            if (qy / kDetTH == y / kDetTH && qx / kDetTW == x / kDetTW) continue;      // the tile kernel did it
            const int q = qy * fnx + qx;
            if (rt::atomic_load_i32(L + q)) det_union(L, p, q, err);
        }
    }
    if (err) rt::atomic_max_i32(status, 1);
}

// ---------------------------------------------------------------------------
// (b) compression + the counts of (c): R[p] = root of p + 1 (0 = background), cnt[root] = pixels.  Integer
// atomics, so the counts do not depend on the order; runs of one root inside a thread's 4 pixels add once.
// ---------------------------------------------------------------------------
SPX_TKERNEL(256)
void detect_compress_kernel(const int32_t* __restrict__ L, int npix, int32_t* __restrict__ R,
                            int32_t* __restrict__ cnt, int32_t* __restrict__ status) {
    const int64_t total = ((int64_t)npix + 3) / 4;
    const int64_t step = rt::grid_size() * 256;
    int err = 0;
    for (int64_t i = rt::block_id() * 256 + rt::thread_id(); i < total; i += step) {
        int run_root = -1, run_n = 0;
        for (int e = 0; e < 4; ++e) {
            const int64_t p = 4 * i + e;
            if (p >= npix) break;
            const int root = L[p] ? det_find(L, (int)p, err) : -1;
            R[p] = root + 1;
            if (root == run_root) { ++run_n; continue; }
            if (run_root >= 0) rt::atomic_add_i32(cnt + run_root, run_n);
            run_root = root;
            run_n = 1;
        }
        if (run_root >= 0) rt::atomic_add_i32(cnt + run_root, run_n);
    }
    if (err) rt::atomic_max_i32(status, 1);
}

// ---------------------------------------------------------------------------
// (c) numbering.  A pixel p is a surviving root when R[p] == p + 1 and cnt[p] >= min_area; survivors are
// numbered 1..L in raster order by an exclusive scan of that flag: per-chunk sums, a scan of the sums by one
// workgroup, then the scan inside each chunk.  Afterwards cnt[root] = new label (0 for an erased root).
// ---------------------------------------------------------------------------
SPX_DEVICE int det_flag(const int32_t* R, const int32_t* cnt, int64_t p, int npix, int min_area) {
    return p < npix && R[p] == (int32_t)(p + 1) && cnt[p] >= min_area;
}

// exclusive scan of one int per thread over the workgroup; s: LDS int[512]; total = sum over the workgroup
SPX_DEVICE int det_block_exscan(int* s, int v, int& total) {
    const int tid = rt::thread_id();
    int* a = s;
    int* b = s + 256;
    a[tid] = v;
    rt::block_sync();
    for (int off = 1; off < 256; off <<= 1) {
        b[tid] = a[tid] + (tid >= off ? a[tid - off] : 0);
        rt::block_sync();
        int* t = a; a = b; b = t;
    }
    const int incl = a[tid];
    total = a[255];
    rt::block_sync();
    return incl - v;
}
constexpr size_t kDetScanLdsBytes = 512 * 4;

SPX_TKERNEL(256)
void detect_flag_count_kernel(const int32_t* __restrict__ R, const int32_t* __restrict__ cnt, int npix,
                              int min_area, int32_t* __restrict__ chunk_sum) {
    SPX_DYN_LDS(lds_raw);
    int* s = reinterpret_cast<int*>(lds_raw);
    const int64_t nchunks = ((int64_t)npix + kDetChunk - 1) / kDetChunk;
    for (int64_t c = rt::block_id(); c < nchunks; c += rt::grid_size()) {
        const int64_t p0 = c * kDetChunk + 4 * rt::thread_id();
        int n = 0;
        for (int e = 0; e < 4; ++e) n += det_flag(R, cnt, p0 + e, npix, min_area);
        int total;
        (void)det_block_exscan(s, n, total);
        if (rt::thread_id() == 0) chunk_sum[c] = total;
    }
}

// one workgroup: chunk_sum -> its exclusive prefix, in place; out_nlabels = the total, or -1 when a merge
// kernel raised the status word
SPX_TKERNEL(256)
void detect_scan_blocks_kernel(int32_t* __restrict__ chunk_sum, int64_t nchunks, const int32_t* __restrict__ status,
                               int32_t* __restrict__ out_nlabels) {
    SPX_DYN_LDS(lds_raw);
    int* s = reinterpret_cast<int*>(lds_raw);
    int carry = 0;
    for (int64_t base = 0; base < nchunks; base += 256) {
        const int64_t c = base + rt::thread_id();
        const int v = c < nchunks ? chunk_sum[c] : 0;
        int total;
        const int ex = det_block_exscan(s, v, total);
        if (c < nchunks) chunk_sum[c] = carry + ex;
        carry += total;
    }
    if (rt::thread_id() == 0) *out_nlabels = *status ? -1 : carry;
}

SPX_TKERNEL(256)
void detect_assign_kernel(const int32_t* __restrict__ R, int32_t* __restrict__ cnt, int npix, int min_area,
                          const int32_t* __restrict__ chunk_sum) {
    SPX_DYN_LDS(lds_raw);
    int* s = reinterpret_cast<int*>(lds_raw);
    const int64_t nchunks = ((int64_t)npix + kDetChunk - 1) / kDetChunk;
    for (int64_t c = rt::block_id(); c < nchunks; c += rt::grid_size()) {
        const int64_t p0 = c * kDetChunk + 4 * rt::thread_id();
        int flag[4], n = 0;
        for (int e = 0; e < 4; ++e) n += flag[e] = det_flag(R, cnt, p0 + e, npix, min_area);
        int total;
        int id = chunk_sum[c] + det_block_exscan(s, n, total);
        for (int e = 0; e < 4; ++e) {
            const int64_t p = p0 + e;
            if (p >= npix) break;
            if (flag[e]) cnt[p] = ++id;
            else if (R[p] == (int32_t)(p + 1)) cnt[p] = 0;          // a root below min_area: erased
        }
    }
}

SPX_TKERNEL(256)
void detect_relabel_kernel(const int32_t* __restrict__ R, const int32_t* __restrict__ cnt, int npix,
                           int32_t* __restrict__ labels) {
    const int64_t step = rt::grid_size() * 256;
    for (int64_t p = rt::block_id() * 256 + rt::thread_id(); p < npix; p += step) {
        const int r = R[p];
        labels[p] = r ? cnt[r - 1] : 0;
    }
}

// ---------------------------------------------------------------------------
// (d) measurements.  One workgroup per label over the label's bounding box boxes[l] = (xmin, ymin, xmax,
// ymax) (spx_label_bboxes_i32's table, row = label).  With w = v - bkg (float64) over the label's pixels and
// dx, dy counted from the box's corner:
//   npix, flux = sum w, x = xmin + sum(w dx)/flux, y = ymin + sum(w dy)/flux        (0-based pixel centres)
//   x2 = sum(w dx^2)/flux - (sum(w dx)/flux)^2, y2 likewise, xy = sum(w dx dy)/flux - mx my
//   a^2, b^2 = (x2 + y2)/2 +- sqrt(((x2 - y2)/2)^2 + xy^2)   (clamped at 0),  theta = atan2(2 xy, x2 - y2)/2 in
//   degrees: the second-moment ellipse of the SExtractor manual, "Position and shape parameters derived
//   from the isophotal profile" (A_IMAGE, B_IMAGE, THETA_IMAGE), restated; the 1/12 px^2 guard SExtractor's
//   source adds to singular moments is NOT applied.
//   peak = max w, (xpeak, ypeak) = its first position in raster order.
//   flags: bit 0 the box touches the frame border, bit 1 flux <= 0 or not finite (then x, y, the moments and
//   the ellipse are NaN), bit 2 a masked or non-finite pixel lies inside the box (such a pixel is never
//   summed, whatever its label).
// Every sum is float64 in a FIXED order -- thread t takes box pixels t, t + 256, ... in turn, then a
// butterfly over the wave's lanes, then waves 0..3 in turn -- so results are bit-identical from run to run.
// table row l - 1 = (npix, flux, x, y, x2, y2, xy, a, b, theta, peak, xpeak, ypeak).
// ---------------------------------------------------------------------------
SPX_DEVICE void measure_finish(const double* S, int npix, int anybad, double pk, int pki, int xmin, int ymin, int w,
                               int border, double* row, int32_t* flag) {
#pragma clang fp contract(off)
    const double nan = __builtin_nan("");
    const double flux = S[0];
    int fl = (border ? 1 : 0) | (anybad ? 4 : 0);
    double x = nan, y = nan, x2 = nan, y2 = nan, xy = nan, a = nan, b = nan, th = nan;
    if (flux > 0.0 && flux - flux == 0.0) {
        const double mx = S[1] / flux, my = S[2] / flux;
        x = (double)xmin + mx;
        y = (double)ymin + my;
        x2 = S[3] / flux - mx * mx;
        y2 = S[4] / flux - my * my;
        xy = S[5] / flux - mx * my;
        const double hs = 0.5 * (x2 + y2), hd = 0.5 * (x2 - y2);
        const double rad = sqrt(hd * hd + xy * xy);
        const double a2 = hs + rad, b2 = hs - rad;
        a = sqrt(a2 > 0.0 ? a2 : 0.0);
        b = sqrt(b2 > 0.0 ? b2 : 0.0);
        th = 0.5 * atan2(2.0 * xy, x2 - y2) * (180.0 / 3.14159265358979323846);
    } else {
        fl |= 2;
    }
    row[0] = (double)npix;
    row[1] = flux;
    row[2] = x; row[3] = y; row[4] = x2; row[5] = y2; row[6] = xy; row[7] = a; row[8] = b; row[9] = th;
    row[10] = npix ? pk : nan;
    row[11] = npix ? (double)(xmin + pki % w) : nan;
    row[12] = npix ? (double)(ymin + pki / w) : nan;
    *flag = fl;
}

template <typename T>
SPX_TKERNEL(256)
void measure_labels_kernel(const T* __restrict__ frame, const uint8_t* __restrict__ bad, double bkg_scalar,
                           const T* __restrict__ bkg_map, const int32_t* __restrict__ labels, int fny, int fnx,
                           int nlabels, const int32_t* __restrict__ boxes, double* __restrict__ table,
                           int32_t* __restrict__ flags) {
    SPX_DYN_LDS(lds_raw);
    double* red_d = reinterpret_cast<double*>(lds_raw);          // [4][7]
    int* red_i = reinterpret_cast<int*>(red_d + 28);             // [4][3]
    const int tid = rt::thread_id();
    for (int64_t lb = rt::block_id(); lb < nlabels; lb += rt::grid_size()) {
        const int l = (int)lb + 1;
        const int xmin = boxes[4 * l], ymin = boxes[4 * l + 1], xmax = boxes[4 * l + 2], ymax = boxes[4 * l + 3];
        const bool empty = xmax < xmin || ymax < ymin || xmin < 0 || ymin < 0 || xmax >= fnx || ymax >= fny;
        const int w = empty ? 1 : xmax - xmin + 1, h = empty ? 0 : ymax - ymin + 1;
        const int64_t n = (int64_t)w * h;
        double S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        double pk = -__builtin_inf();
        int pki = 0x7fffffff, npix = 0, anybad = 0;
        for (int64_t i = tid; i < n; i += 256) {
            const int yy = (int)(i / w), xx = (int)(i - (int64_t)yy * w);
            const int64_t p = (int64_t)(ymin + yy) * fnx + xmin + xx;
            const T v = frame[p];
            if (!(v - v == T(0)) || (bad && bad[p])) {
                anybad = 1;
                continue;
            }
            if (labels[p] != l) continue;
            const double wv = (double)v - (bkg_map ? (double)bkg_map[p] : bkg_scalar);
            const double dx = (double)xx, dy = (double)yy;
            S[0] += wv;
            S[1] += wv * dx;
            S[2] += wv * dy;
            S[3] += wv * (dx * dx);
            S[4] += wv * (dy * dy);
            S[5] += wv * (dx * dy);
            ++npix;
            if (wv > pk) { pk = wv; pki = (int)i; }
        }
        for (int m = 32; m >= 1; m >>= 1) {
            for (int k = 0; k < 6; ++k) S[k] += rt::shfl_xor(S[k], m);
            npix += rt::shfl_xor(npix, m);
            anybad |= rt::shfl_xor(anybad, m);
            const double opk = rt::shfl_xor(pk, m);
            const int opi = rt::shfl_xor(pki, m);
            if (opk > pk || (opk == pk && opi < pki)) { pk = opk; pki = opi; }
        }
        if ((tid & 63) == 0) {
            const int wv = tid >> 6;
            for (int k = 0; k < 6; ++k) red_d[wv * 7 + k] = S[k];
            red_d[wv * 7 + 6] = pk;
            red_i[wv * 3] = npix; red_i[wv * 3 + 1] = anybad; red_i[wv * 3 + 2] = pki;
        }
        rt::block_sync();
        if (tid == 0) {
            for (int wv = 1; wv < 4; ++wv) {
                for (int k = 0; k < 6; ++k) S[k] += red_d[wv * 7 + k];
                npix += red_i[wv * 3];
                anybad |= red_i[wv * 3 + 1];
                const double opk = red_d[wv * 7 + 6];
                const int opi = red_i[wv * 3 + 2];
                if (opk > pk || (opk == pk && opi < pki)) { pk = opk; pki = opi; }
            }
            const int border = !empty && (xmin == 0 || ymin == 0 || xmax == fnx - 1 || ymax == fny - 1);
            measure_finish(S, npix, anybad, pk, npix ? pki : 0, xmin, ymin, w, border,
                           table + (int64_t)lb * kMeasureCols, flags + lb);
        }
        rt::block_sync();
    }
}
constexpr size_t kMeasureLdsBytes = 28 * 8 + 12 * 4;

}  // namespace spx
