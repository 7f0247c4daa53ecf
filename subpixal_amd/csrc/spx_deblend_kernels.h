// spx_deblend_kernels.h -- deblending of merged sources: a multi-threshold tree per detected segment and a
// level-by-level flood from the branches that count, in the spirit of SExtractor's DEBLEND_NTHRESH /
// DEBLEND_MINCONT.  SExtractor's own tree is unpinned (no binary, no fixtures): the definition is this
// library's, and tests/deblend_statement.py restates it in numpy/scipy with EXACT equality.
//   deblend_parents_kernel  one workgroup per parent (label) over the parent's bounding box: quantise, walk the
//                           levels downward (incremental union-find, per-root flux / count / significant
//                           children / has-objects), seed, flood, write every final segment as R[p] = first
//                           pixel of the segment + 1 into the frame-sized R of the numbering kernels
//   deblend_table_kernel    out_parent / out_dflags per final segment, after detect_flag_count / scan_blocks /
//                           assign / relabel (spx_detect_kernels.h) numbered the segments 1..L'
// Needs spx_rt_hip.h (or the CPU harness) and spx_detect_kernels.h first.  Plain C++ and vector atomics only.
//
// DEFINITION.  include/subpixal_hip.h (the block above spx_deblend_labels_*) is the normative text; this is the
// same definition in the kernel's terms, kept beside the code that implements it, step for step.
//   f = the filtered image of spx_detect_label_* (the same fused multiply-add chain in the frame's dtype, v' = 0
//   outside the frame and at masked or non-finite pixels; without a filter f = v'), converted exactly to
//   float64.  Per parent P = the pixels of one label l in 1..nlabels inside boxes[l] (other labels inside the
//   box are ignored everywhere):
//   1. lo = min f, hi = max f over P; hi <= lo: the parent is left whole.
//      q(p) = min(2^30, floor(((f(p) - lo) / (hi - lo)) * 2^30)), an integer; float64, every operation rounded
//      on its own (no contraction).  F(X) = sum of q over X, an exact 64-bit integer.
//   2. TQ_0 = 0.  mode 0 (exponential) with lo > 0 and rho = hi / lo finite: g = rho under log2(n + 1) square
//      roots, p_0 = 1, p_k = p_(k-1) * g, x_k = ((p_k - 1) / (rho - 1)) * 2^30, TQ_k = min(2^30, ceil(x_k)),
//      k = 1..n.  mode 1 (linear) and every other case of mode 0: TQ_k = k * 2^30 / (n + 1).  float64, each step
//      rounded on its own, only + - * / sqrt.  S_k = {p in P : q(p) >= TQ_k}; S_0 = P.
//   3. Tree, k = n down to 0.  The children of a connected component C of S_k (the detection's connectivity)
//      are the components of S_(k+1) inside C.  A child D is significant when objs(D) is not empty, or when
//      (double)F(D) >= c * (double)F(P) and |D| >= min_area.  Two or more significant children: objs(C) = the
//      union over the significant children of objs(D) if that is not empty, else {D}.  Otherwise objs(C) = the
//      (at most one) non-empty objs(D) among its children, or empty; in the empty case C goes on as ONE
//      candidate, insignificant bumps included.  No component of S_0 with objects: the parent is left whole.
//      Otherwise the members of the objs of S_0's components are the seeds, numbered 1..m in raster order of
//      each seed's first pixel.
//   4. Flood.  o(p) = seed number on seed pixels, 0 elsewhere.  For k = n down to 0, synchronous sweeps until
//      one changes nothing: every p in P with o(p) = 0 and q(p) >= TQ_k that has a neighbour (same
//      connectivity) with o > 0 IN THE PREVIOUS SWEEP'S STATE takes the o of the neighbour with the largest q;
//      ties go to the smallest o.  All of a connected P ends up assigned (pixels of a parent that is not
//      connected under that connectivity and that no seed can reach stay together as one further child).
//   5. Parents whose box holds more than kDebMaxBoxPixels (65536) pixels are left whole and flagged.
//   Every final segment (children and untouched parents) is numbered 1..L' in raster order of its first pixel.
//
// HOW.  Every comparison after step 1 is on integers, every sum an integer atomic: results do not depend on
// the schedule, the grid or the storage.  Roots are first pixels (det_union links the larger root below the
// smaller), so a seed's first pixel IS its root index and "ties to the smallest o" compares root indices.
// One level = four phases between workgroup barriers:
//   A  every active pixel notes whether the component D it is in now is a candidate (significant, no objects),
//      every root notes its significance; the level's new pixels become active singletons
//   B  new pixels join their active neighbours (det_union)
//   C  every former root and every new pixel adds flux, count, significance, has-objects to its root of now;
//      every pixel notes that root
//   D  roots with two or more significant children: the candidates below them become seeds; has-objects set;
//      every link now points at the root
// A level whose threshold equals the next one's has no new pixel and is skipped.  The flood is a propose /
// commit sweep pair between barriers; a sweep that proposes nothing ends its level.  Every loop ends by
// construction; chains are guarded by det_find / det_union's status word.  No workgroup waits for another.
//
// STORAGE: 36 B per box pixel (kDebBytesPerPixel: flux u64, q, link, count, nsig, state, o, cand as int32; int32
// links because det_find / det_union are reused as they are), the same device functions over pointers into LDS
// or into a slot of the global workspace.  THE CUT:
//   boxes of     0 .. 256   pixels  one WAVE per parent (64 threads, 10 KiB of LDS; hipcc emits no s_barrier for
//                                   a one-wave workgroup, so the barriers of a level cost nothing)
//   boxes of   257 .. 1024  pixels  256 threads, 37 KiB of LDS: four workgroups per CU
//   boxes of  1025 .. 2048  pixels  256 threads, 73 KiB of LDS: two workgroups per CU
//   boxes of  2049 .. 65536 pixels  1024 threads (latency cover), one of kDebSlots workspace slots per workgroup
//   larger boxes                    streamed through as they are, flag 16
// Each class is one launch of the same kernel over ALL labels; a workgroup skips the labels of other classes.
// Links are compressed once per level (phase C notes every pixel's root, phase D stores it), so the finds of
// phases A and C stay one or two hops.
#pragma once

namespace spx {

constexpr int kDebMaxBoxPixels = 65536;
constexpr int kDebWavePixels = 256;              // up to here: one wave per parent
constexpr int kDebMidPixels = 1024;              // up to here: 256 threads, four workgroups per CU
constexpr int kDebLdsPixels = 2048;              // up to here: per-pixel state in LDS (two workgroups per CU)
constexpr int kDebWsThreads = 1024;              // workgroup of the global-memory class: latency cover
constexpr int kDebBytesPerPixel = 36;
constexpr int kDebSlots = 64;                    // workgroups (= workspace slots) of the global-memory class
constexpr int kDebHeadBytes = 1024;              // LDS header: levels, scalars, reduction slots, filter
constexpr int kDebFlagChild = 8, kDebFlagNoDeblend = 16;
constexpr int kDebIdMask = 0x1ffff;              // cand: candidate id (root + 1 <= 65536) | the bits below
constexpr int kDebWasRoot = 1 << 30, kDebSig = 1 << 29, kDebObj = 1 << 28;

constexpr size_t deb_lds_bytes(int pixels) { return (size_t)kDebHeadBytes + (size_t)pixels * kDebBytesPerPixel; }

struct DebHead {                                 // at the start of the dynamic LDS (<= kDebHeadBytes)
    int32_t tq[66];                              // TQ_0..TQ_n, then INT_MAX
    int32_t first, rest_first, changed[2], any_seed, pad;
    unsigned long long flux;                     // F(P)
    double red[32];                              // min / max per wave (up to 16 waves)
    double filt[49];                             // the filter, in the frame's dtype (float uses the front half)
};
static_assert(sizeof(DebHead) <= kDebHeadBytes, "LDS header");

struct DebState {
    unsigned long long* F;
    int32_t *q, *L, *cnt, *nsig, *st, *o, *cand;
};
SPX_DEVICE DebState deb_state(unsigned char* base, int pixels) {
    DebState s;
    s.F = reinterpret_cast<unsigned long long*>(base);
    s.q = reinterpret_cast<int32_t*>(s.F + pixels);
    s.L = s.q + pixels;
    s.cnt = s.L + pixels;
    s.nsig = s.cnt + pixels;
    s.st = s.nsig + pixels;
    s.o = s.st + pixels;
    s.cand = s.o + pixels;
    return s;
}

// v' of the definition at frame position (gy, gx)
template <typename T>
SPX_DEVICE T deb_vprime(const T* frame, const uint8_t* bad, int fny, int fnx, int gy, int gx) {
    if (gy < 0 || gy >= fny || gx < 0 || gx >= fnx) return T(0);
    const int64_t g = (int64_t)gy * fnx + gx;
    const T v = frame[g];
    return ((v - v == T(0)) && !(bad && bad[g])) ? v : T(0);
}

SPX_DEVICE int deb_quantise(double f, double lo, double hi) {
#pragma clang fp contract(off)
    const double two30 = 1073741824.0;
    const double t = floor(((f - lo) / (hi - lo)) * two30);
    return !(t > 0.0) ? 0 : (t < two30 ? (int)t : 1 << 30);
}

// step 2, by one thread
SPX_DEVICE void deb_levels(double lo, double hi, int n, int mode, int32_t* tq) {
#pragma clang fp contract(off)
    const double two30 = 1073741824.0;
    tq[0] = 0;
    tq[n + 1] = 0x7fffffff;
    double rho = 0.0;
    bool expo = false;
    if (mode == 0 && lo > 0.0) {
        rho = hi / lo;
        expo = rho - rho == 0.0;
    }
    if (expo) {
        double g = rho;
        for (int m = n + 1; m > 1; m >>= 1) g = sqrt(g);
        double p = 1.0;
        for (int k = 1; k <= n; ++k) {
            p = p * g;
            const double x = ((p - 1.0) / (rho - 1.0)) * two30;
            tq[k] = !(x < two30) ? 1 << 30 : (int)ceil(x);
        }
    } else {
        for (int k = 1; k <= n; ++k) tq[k] = (int)(((int64_t)k << 30) / (n + 1));
    }
}

SPX_DEVICE bool deb_significant(const DebState& s, int r, double cflux, int min_area) {
    return (s.st[r] & 1) || ((double)s.F[r] >= cflux && s.cnt[r] >= min_area);
}

// ---------------------------------------------------------------------------
// One workgroup of NT threads per parent whose box holds nmin..nmax pixels (nmax >= kDebMaxBoxPixels: and
// every larger one, left whole).  WS: per-pixel state in slot block_id() of `slots` instead of LDS.
// Writes R (frame-sized, zeroed before) and cnt at segment roots, pflag[l] = 0 / 8 / 16.
// ---------------------------------------------------------------------------
template <typename T, int NT, bool WS>
SPX_TKERNEL(NT)
void deblend_parents_kernel(const T* __restrict__ frame, const uint8_t* __restrict__ bad, const T* __restrict__ filt,
                            int fky, int fkx, int fny, int fnx, const int32_t* __restrict__ labels, int nlabels,
                            const int32_t* __restrict__ boxes, int conn, int min_area, int nlev, double contrast,
                            int mode, int nmin, int nmax, unsigned char* __restrict__ slots, size_t slot_bytes,
                            int32_t* __restrict__ R, int32_t* __restrict__ cnt, int32_t* __restrict__ pflag,
                            int32_t* __restrict__ status) {
    SPX_DYN_LDS(lds_raw);
    DebHead* hd = reinterpret_cast<DebHead*>(lds_raw);
    const int tid = rt::thread_id();
    const int hy = fky / 2, hx = fkx / 2;
    const int nnb = conn == 8 ? 8 : 4;
    int err = 0;
    T* fk = reinterpret_cast<T*>(hd->filt);
    if (filt && tid < fky * fkx) fk[tid] = filt[tid];
    for (int64_t lb = rt::block_id(); lb < nlabels; lb += rt::grid_size()) {
        const int l = (int)lb + 1;
        const int xmin = boxes[4 * l], ymin = boxes[4 * l + 1], xmax = boxes[4 * l + 2], ymax = boxes[4 * l + 3];
        const bool empty = xmax < xmin || ymax < ymin || xmin < 0 || ymin < 0 || xmax >= fnx || ymax >= fny;
        const int w = empty ? 1 : xmax - xmin + 1, h = empty ? 0 : ymax - ymin + 1;
        const int64_t n64 = (int64_t)w * h;
        if (n64 < nmin || (n64 > nmax && nmax < kDebMaxBoxPixels)) continue;      // another launch's parent
        rt::block_sync();                                                        // the header is free again
        if (tid == 0) {
            hd->first = 0x7fffffff;
            hd->rest_first = 0x7fffffff;
            hd->changed[0] = hd->changed[1] = 0;
            hd->any_seed = 0;
            hd->flux = 0;
        }
        rt::block_sync();
        if (n64 > kDebMaxBoxPixels) {
            // over the limit: the parent as it is.  Its first pixel, then R
            int mine = 0x7fffffff;
            for (int64_t i = tid; i < n64; i += NT) {
                const int yy = (int)(i / w), xx = (int)(i - (int64_t)yy * w);
                const int64_t p = (int64_t)(ymin + yy) * fnx + xmin + xx;
                if (labels[p] == l && p < mine) mine = (int)p;
            }
            if (mine != 0x7fffffff) rt::atomic_min_i32(&hd->first, mine);
            rt::block_sync();
            const int first = hd->first;
            for (int64_t i = tid; i < n64; i += NT) {
                const int yy = (int)(i / w), xx = (int)(i - (int64_t)yy * w);
                const int64_t p = (int64_t)(ymin + yy) * fnx + xmin + xx;
                if (labels[p] == l) R[p] = first + 1;
            }
            if (tid == 0) {
                if (first != 0x7fffffff) cnt[first] = 1;
                pflag[l] = kDebFlagNoDeblend;
            }
            continue;
        }
        const int N = (int)n64;
        const DebState s = deb_state(WS ? slots + (size_t)rt::block_id() * slot_bytes : lds_raw + kDebHeadBytes,
                                     WS ? (int)(slot_bytes / kDebBytesPerPixel) : nmax);
        // ---- step 1: f, lo, hi, q
        double lo = __builtin_inf(), hi = -__builtin_inf();
        for (int i = tid; i < N; i += NT) {
            const int yy = i / w, xx = i - yy * w;
            const int gy = ymin + yy, gx = xmin + xx;
            s.o[i] = 0;
            s.L[i] = 0;
            if (labels[(int64_t)gy * fnx + gx] != l) {
                s.q[i] = -1;
                continue;
            }
            s.q[i] = 0;
            T f;
            if (filt)
                f = det_filter_chain<T>(fk, fky, fkx, [&](int j, int k) {
                    return deb_vprime(frame, bad, fny, fnx, gy + j - hy, gx + k - hx);
                });
            else
                f = deb_vprime(frame, bad, fny, fnx, gy, gx);
            const double fd = (double)f;
            s.F[i] = __builtin_bit_cast(unsigned long long, fd);          // parked here until q is known
            lo = fd < lo ? fd : lo;
            hi = fd > hi ? fd : hi;
            rt::atomic_min_i32(&hd->first, i);
        }
        for (int m = 32; m >= 1; m >>= 1) {
            const double a = rt::shfl_xor(lo, m), b = rt::shfl_xor(hi, m);
            lo = a < lo ? a : lo;
            hi = b > hi ? b : hi;
        }
        if ((tid & 63) == 0) {
            hd->red[2 * (tid >> 6)] = lo;
            hd->red[2 * (tid >> 6) + 1] = hi;
        }
        rt::block_sync();
        for (int wv = 0; wv < NT / 64; ++wv) {
            const double a = hd->red[2 * wv], b = hd->red[2 * wv + 1];
            lo = a < lo ? a : lo;
            hi = b > hi ? b : hi;
        }
        const int first = hd->first;                 // box-local index of P's first pixel
        bool split = false;
        if (first != 0x7fffffff && hi > lo) {
            if (tid == 0) deb_levels(lo, hi, nlev, mode, hd->tq);
            unsigned long long part = 0;
            for (int i = tid; i < N; i += NT) {
                if (s.q[i] < 0) continue;
                const int q = deb_quantise(__builtin_bit_cast(double, s.F[i]), lo, hi);
                s.q[i] = q;
                part += (unsigned long long)q;
            }
            if (part) rt::atomic_accum_u64(&hd->flux, part);
            rt::block_sync();
            const double cflux = contrast * (double)hd->flux;
            // ---- step 3: the tree
            for (int k = nlev; k >= 0; --k) {
                const int tlo = hd->tq[k], thi = hd->tq[k + 1];
                if (tlo == thi) continue;
                for (int i = tid; i < N; i += NT) {                               // A
                    int c = 0;
                    if (s.L[i]) {
                        const int r = det_find(s.L, i, err);
                        const bool ho = s.st[r] & 1;
                        const bool sg = deb_significant(s, r, cflux, min_area);
                        c = (sg && !ho) ? r + 1 : 0;
                        if (r == i) c |= kDebWasRoot | (sg ? kDebSig : 0) | (ho ? kDebObj : 0);
                    }
                    s.cand[i] = c;
                    s.nsig[i] = 0;
                    const int q = s.q[i];
                    if (q >= tlo && q < thi) {          // not active yet: no chain leads here, nobody reads it
                        s.F[i] = (unsigned long long)q;
                        s.cnt[i] = 1;
                        s.st[i] = 0;
                        s.L[i] = i + 1;
                    }
                }
                rt::block_sync();
                for (int i = tid; i < N; i += NT) {                               // B
                    const int q = s.q[i];
                    if (q < tlo || q >= thi) continue;
                    const int yy = i / w, xx = i - yy * w;
                    for (int nb = 0; nb < nnb; ++nb) {
                        const int dy = nb < 4 ? (nb == 1 ? -1 : (nb == 2 ? 1 : 0)) : (nb < 6 ? -1 : 1);
                        const int dx = nb < 4 ? (nb == 0 ? -1 : (nb == 3 ? 1 : 0)) : ((nb & 1) ? 1 : -1);
                        const int y2 = yy + dy, x2 = xx + dx;
                        if (y2 < 0 || y2 >= h || x2 < 0 || x2 >= w) continue;
                        const int j = y2 * w + x2;
                        if (rt::atomic_load_i32(s.L + j)) det_union(s.L, i, j, err);
                    }
                }
                rt::block_sync();
                for (int i = tid; i < N; i += NT) {                               // C
                    if (!s.L[i]) continue;
                    const int q = s.q[i], c = s.cand[i];
                    const bool fresh = q >= tlo && q < thi;
                    const int r = det_find(s.L, i, err);
                    if (r != i) s.nsig[i] = r;          // a non-root's slot is free: its root, for phase D
                    if (!fresh && !(c & kDebWasRoot)) continue;
                    if (r != i) {
                        rt::atomic_accum_u64(s.F + r, s.F[i]);
                        rt::atomic_add_i32(s.cnt + r, s.cnt[i]);
                    }
                    if (c & kDebSig) rt::atomic_add_i32(s.nsig + r, 1);
                    if (c & kDebObj) rt::atomic_or_i32(s.st + r, 4);
                }
                rt::block_sync();
                bool seeded = false;
                for (int i = tid; i < N; i += NT) {                               // D
                    const int li = s.L[i];
                    if (!li) continue;
                    const int r = li == i + 1 ? i : s.nsig[i];
                    const int ns = s.nsig[r], c = s.cand[i] & kDebIdMask;
                    if (ns >= 2 && c) {
                        s.o[i] = c;
                        seeded = true;
                    }
                    if (r == i) s.st[i] = (ns >= 2 || (s.st[i] & 4)) ? 1 : 0;
                    else s.L[i] = r + 1;                // compressed: nobody follows links in this phase
                }
                if (seeded) rt::atomic_or_i32(&hd->any_seed, 1);
                rt::block_sync();
            }
            split = hd->any_seed != 0;
            if (split) {
                // ---- step 4: the flood; cand holds the proposals
                int sweep = 0;
                for (int k = nlev; k >= 0; --k) {
                    const int tlo = hd->tq[k];
                    if (tlo == hd->tq[k + 1]) continue;
                    for (;;) {
                        bool any = false;
                        for (int i = tid; i < N; i += NT) {
                            int best = 0;
                            if (s.o[i] == 0 && s.q[i] >= tlo) {
                                const int yy = i / w, xx = i - yy * w;
                                int bq = -1;
                                for (int nb = 0; nb < nnb; ++nb) {
                                    const int dy = nb < 4 ? (nb == 1 ? -1 : (nb == 2 ? 1 : 0)) : (nb < 6 ? -1 : 1);
                                    const int dx = nb < 4 ? (nb == 0 ? -1 : (nb == 3 ? 1 : 0)) : ((nb & 1) ? 1 : -1);
                                    const int y2 = yy + dy, x2 = xx + dx;
                                    if (y2 < 0 || y2 >= h || x2 < 0 || x2 >= w) continue;
                                    const int j = y2 * w + x2;
                                    const int oj = s.o[j];
                                    if (!oj) continue;
                                    const int qj = s.q[j];
                                    if (qj > bq || (qj == bq && oj < best)) {
                                        bq = qj;
                                        best = oj;
                                    }
                                }
                            }
                            s.cand[i] = best;
                            any |= best != 0;
                        }
                        if (any) rt::atomic_or_i32(&hd->changed[sweep & 1], 1);
                        rt::block_sync();
                        const int ch = hd->changed[sweep & 1];
                        if (tid == 0) hd->changed[(sweep + 1) & 1] = 0;
                        if (ch)
                            for (int i = tid; i < N; i += NT)
                                if (s.cand[i]) s.o[i] = s.cand[i];
                        rt::block_sync();
                        ++sweep;
                        if (!ch) break;
                    }
                }
                // first pixel of every child (nsig by seed root; the unreached rest in the header)
                for (int i = tid; i < N; i += NT) s.nsig[i] = 0x7fffffff;
                rt::block_sync();
                for (int i = tid; i < N; i += NT) {
                    if (s.q[i] < 0) continue;
                    const int o = s.o[i];
                    rt::atomic_min_i32(o ? s.nsig + (o - 1) : &hd->rest_first, i);
                }
                rt::block_sync();
            }
        }
        for (int i = tid; i < N; i += NT) {
            if (s.q[i] < 0) continue;
            int fi = first;
            if (split) {
                const int o = s.o[i];
                fi = o ? s.nsig[o - 1] : hd->rest_first;
            }
            const int yy = i / w, xx = i - yy * w;
            const int fy = fi / w, fx = fi - fy * w;
            const int gfirst = (ymin + fy) * fnx + xmin + fx;
            R[(int64_t)(ymin + yy) * fnx + xmin + xx] = gfirst + 1;
            if (i == fi) cnt[gfirst] = 1;
        }
        if (tid == 0) pflag[l] = split ? kDebFlagChild : 0;
    }
    if (err) rt::atomic_max_i32(status, 1);
}

// after the numbering (cnt[first pixel] = the segment's number): one row per final segment
SPX_TKERNEL(256)
void deblend_table_kernel(const int32_t* __restrict__ R, const int32_t* __restrict__ cnt,
                          const int32_t* __restrict__ labels, const int32_t* __restrict__ pflag, int npix,
                          int nlabels, int max_out, int32_t* __restrict__ out_parent,
                          int32_t* __restrict__ out_dflags) {
    const int64_t step = rt::grid_size() * 256;
    for (int64_t p = rt::block_id() * 256 + rt::thread_id(); p < npix; p += step) {
        if (R[p] != (int32_t)(p + 1)) continue;
        const int seg = cnt[p], l = labels[p];
        if (seg < 1 || seg > max_out || l < 1 || l > nlabels) continue;
        out_parent[seg - 1] = l;
        out_dflags[seg - 1] = pflag[l];
    }
}

}  // namespace spx
