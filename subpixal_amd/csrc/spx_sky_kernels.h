// spx_sky_kernels.h -- sigma-clipped statistics of WHOLE frames on the device: the sky level the drizzle subtracts
// (resample.DeviceDrizzle, skysub=True).  The mesh statistics of spx_background_kernels.h sort one cell in LDS and
// stop at 16384 pixels; a frame of 4096 x 4096 cannot be sorted there, so the median is found by a streaming radix
// SELECTION over the order-preserving integer key of the values and the moments by a fixed-order float64 sum.
//   sky_init_kernel          the per-frame state record: hard bounds, shape check
//   sky_hist_kernel<T>       one digit of the keys inside the range that match the prefix found so far: LDS
//                            histogram per workgroup (integer atomics), flushed to the frame's global histogram
//   sky_select_kernel<T>     one workgroup per frame: round logic (steps 1 and 5 of the definition), the digit that
//                            holds rank (n - 1) / 2 and rank n / 2, the median and the all-equal test after the last digit
//   sky_moments_kernel<T>    S1 = sum(v - med), S2 = sum((v - med)^2) in float64, kSkyMomentGrid partials per frame
//   sky_finish_kernel        adds the partials in slot order: mean, std, steps 4 and 5 (the next candidate range)
//   sky_output_kernel        state -> the caller's tables
// Needs spx_rt_hip.h (or the CPU harness) first.  Plain C++ and vector stores only.
//
// DEFINITION: include/subpixal_hip.h (sky block); tests/sky_statement.py states it again in numpy.
//
// LAUNCH SEQUENCE (host::sky_stats_launch below, shared by spx_capi.hip and tests/cpu_emu/emu_sky.cpp): init, then
// for every round r = 0 .. max_iters: for every digit p = 0 .. D-1 { hist(p); select(p, r) }; moments; finish(r).
// Then output.  D = 3 for float32 (digits of 11, 11, 10 bits), 6 for float64 (five of 11 bits and one of 9).  A frame
// is read D + 1 times per round: (max_iters + 1) (D + 1) reads in all, 24 / 42 for float32 / float64 at max_iters = 5
// (COUNTED from this sequence).  A frame that has stopped (state.done) makes every later workgroup of it return at
// once.  Nothing is copied to the host and no workgroup waits for another: every loop runs over a fixed index range.
//
// REPRODUCIBILITY.  The histograms are integer sums: they do not depend on the order workgroups arrive in, so the
// hist kernel's grid is free (the library sizes it by the CU count, the CPU harness takes a few workgroups).  The
// moments are float64 sums in a FIXED order that is part of the definition: the frame's pixels are numbered
// i = y * nx + x; kSkyMomentGrid = 16 workgroups of 256 threads take a frame, and thread t of workgroup b adds the
// terms of pixels j, j + 4096, j + 8192, ... (j = 256 b + t) in that order, skipping pixels that are not in the
// range; the 64 lanes of a wave are added by a butterfly (partner lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1: s = s + partner's
// s, the same bits in both lanes because the addition commutes); the four wave sums of a workgroup are added in
// wave order starting from 0.0, and sky_finish_kernel adds the 16 workgroup sums in workgroup order starting from 0.0.
// The moment grid is this constant for every device, so the CPU-thread run of this source gives the same bits.
//
// TIES.  A sky frame's values share their leading key bits (one exponent), and a constant frame shares all of them:
// every lane of every wave would hit one LDS bin.  Each thread therefore keeps the bin of its previous value and a
// run count, and issues an LDS atomic only when the bin changes or its pixels end: a thread's pixels are 256 apart
// in a row-major frame, their leading digits agree almost always, and a constant frame costs one LDS atomic per
// thread and pass instead of one per pixel.
#pragma once

namespace spx {

constexpr int kSkyMaxFrames = 128;
constexpr int kSkyBins = 2048;                     // 11-bit digits
constexpr int kSkyMomentGrid = 16;                 // workgroups per frame of sky_moments_kernel: PART OF THE DEFINITION
constexpr int kSkyThreads = 256;
constexpr int kSkyStride = kSkyMomentGrid * kSkyThreads;
constexpr size_t kSkyHistLdsBytes = (size_t)2 * kSkyBins * 4;
constexpr size_t kSkySelectLdsBytes = (size_t)(kSkyThreads + 8) * 8;
constexpr size_t kSkyMomentLdsBytes = 64;
constexpr int kSkyEmpty = 1, kSkyBadFrame = 2;     // SPX_SKY_EMPTY, SPX_SKY_BAD_FRAME
constexpr int kSkyMedian = 0, kSkyMean = 1, kSkyMode = 2;

struct SkyState {                                  // 256 bytes per frame
    double lo, hi;                                 // the current closed range
    double cand_lo, cand_hi;                       // the range the next histogram pass counts (step 5's lo', hi')
    double med, mean, sd;
    unsigned long long prefix[2];                  // key bits found so far of rank (n - 1) / 2 and n / 2
    long long rank[2];                             // their ranks among the values that match the prefix
    long long n_usable, n;
    int32_t same;                                  // both ranks still follow one prefix
    int32_t done, need_moments, rounds, status;
    int32_t pad_[33];
};
static_assert(sizeof(SkyState) == 256, "SkyState is 256 bytes");

// workspace of nframes frames: [nframes] SkyState, [nframes][2][kSkyBins] int32 histograms,
// [nframes][kSkyMomentGrid][2] float64 partial sums
constexpr size_t kSkyFrameBytes = sizeof(SkyState) + (size_t)2 * kSkyBins * 4 + (size_t)kSkyMomentGrid * 16;
SPX_DEVICE SkyState* sky_state(void* work, int f) { return reinterpret_cast<SkyState*>(work) + f; }
SPX_DEVICE int32_t* sky_hist(void* work, int nframes, int f) {
    return reinterpret_cast<int32_t*>(reinterpret_cast<SkyState*>(work) + nframes) + (size_t)f * 2 * kSkyBins;
}
SPX_DEVICE double* sky_partials(void* work, int nframes, int f) {
    return reinterpret_cast<double*>(reinterpret_cast<unsigned char*>(work) +
                                     (size_t)nframes * (sizeof(SkyState) + (size_t)2 * kSkyBins * 4)) +
           (size_t)f * kSkyMomentGrid * 2;
}

// the order-preserving key: -0.0 is counted as +0.0 (v + 0 has the sign bit clear for both)
template <typename T> struct SkyKey;
template <> struct SkyKey<float> {
    static constexpr int digits = 3, bits = 32;
    static SPX_DEVICE unsigned long long of(float v) {
        const unsigned u = __builtin_bit_cast(unsigned, v + 0.0f);
        return (u >> 31) ? (unsigned)~u : (u | 0x80000000u);
    }
    static SPX_DEVICE double value(unsigned long long k) {
        const unsigned q = (unsigned)k;
        const unsigned u = (q >> 31) ? (q & 0x7fffffffu) : ~q;
        return (double)__builtin_bit_cast(float, u);
    }
};
template <> struct SkyKey<double> {
    static constexpr int digits = 6, bits = 64;
    static SPX_DEVICE unsigned long long of(double v) {
        const unsigned long long u = __builtin_bit_cast(unsigned long long, v + 0.0);
        return (u >> 63) ? ~u : (u | (1ull << 63));
    }
    static SPX_DEVICE double value(unsigned long long k) {
        const unsigned long long u = (k >> 63) ? (k & ~(1ull << 63)) : ~k;
        return __builtin_bit_cast(double, u);
    }
};
// digit p of a key of `bits` bits: its shift and width (the last digit takes what is left: 10 or 9 bits)
SPX_DEVICE int sky_digit_shift(int bits, int p) { const int s = bits - 11 * (p + 1); return s > 0 ? s : 0; }
SPX_DEVICE int sky_digit_width(int bits, int p) { const int s = bits - 11 * (p + 1); return s >= 0 ? 11 : 11 + s; }

template <typename T>
SPX_DEVICE bool sky_in_range(const T* __restrict__ frame, const T* __restrict__ weight,
                             const uint8_t* __restrict__ mask, long long i, double lo, double hi, T* out) {
    const T v = frame[i];
    *out = v;
    bool ok = (v - v == T(0)) && (double)v >= lo && (double)v <= hi;
    if (mask) ok = ok && mask[i] == 0;
    if (weight) {
        const T w = weight[i];
        ok = ok && (w - w == T(0)) && w > T(0);
    }
    return ok;
}

// One thread per frame.  lower / upper: NaN = no bound.
SPX_TKERNEL(256)
void sky_init_kernel(const void* const* __restrict__ frames, const int32_t* __restrict__ shapes, int nframes,
                     double lower, double upper, void* __restrict__ work) {
    const int f = rt::thread_id();
    if (rt::block_id() != 0 || f >= nframes) return;
    SkyState* st = sky_state(work, f);
    const double inf = __builtin_inf();
    st->lo = st->cand_lo = lower == lower ? lower : -inf;
    st->hi = st->cand_hi = upper == upper ? upper : inf;
    const double nan = __builtin_nan("");
    st->med = st->mean = st->sd = nan;
    st->prefix[0] = st->prefix[1] = 0;
    st->rank[0] = st->rank[1] = 0;
    st->n_usable = st->n = 0;
    st->same = 1;
    st->need_moments = st->rounds = 0;
    const long long ny = shapes[2 * f], nx = shapes[2 * f + 1];
    const bool bad = !frames[f] || ny < 1 || nx < 1 || ny * nx >= 2147483647LL;
    st->status = bad ? kSkyBadFrame : 0;
    st->done = bad ? 1 : 0;
}

// grid = nframes * gpf workgroups (gpf any number >= 1: the sums are integers), frame = block / gpf.
template <typename T>
SPX_TKERNEL(256)
void sky_hist_kernel(const T* const* __restrict__ frames, const T* const* __restrict__ weights,
                     const uint8_t* const* __restrict__ masks, const int32_t* __restrict__ shapes, int nframes,
                     int gpf, int pass, void* __restrict__ work) {
    SPX_DYN_LDS(lds_raw);
    int* lh = reinterpret_cast<int*>(lds_raw);
    const int tid = rt::thread_id();
    const int f = (int)(rt::block_id() / gpf), b = (int)(rt::block_id() - (int64_t)f * gpf);
    if (f >= nframes) return;
    const SkyState* st = sky_state(work, f);
    if (st->done) return;                                    // the same for every thread of the workgroup
    const long long npix = (long long)shapes[2 * f] * shapes[2 * f + 1];
    if ((long long)b * kSkyThreads >= npix) return;          // nothing to count: nothing to flush
    for (int i = tid; i < 2 * kSkyBins; i += kSkyThreads) lh[i] = 0;
    rt::block_sync_lds();
    const T* frame = frames[f];
    const T* weight = weights ? weights[f] : nullptr;
    const uint8_t* mask = masks ? masks[f] : nullptr;
    const double lo = st->cand_lo, hi = st->cand_hi;
    const int shift = sky_digit_shift(SkyKey<T>::bits, pass), width = sky_digit_width(SkyKey<T>::bits, pass);
    const unsigned long long above = pass == 0 ? 0ull : (~0ull << sky_digit_shift(SkyKey<T>::bits, pass - 1));
    const unsigned long long pa = st->prefix[0], pb = st->prefix[1];
    const bool same = st->same != 0;
    const unsigned dmask = (1u << width) - 1u;
    int run_bin = -1, run = 0;
    for (long long i = (long long)b * kSkyThreads + tid; i < npix; i += (long long)gpf * kSkyThreads) {
        T v;
        if (!sky_in_range(frame, weight, mask, i, lo, hi, &v)) continue;
        const unsigned long long key = SkyKey<T>::of(v);
        int bin = (int)((unsigned)(key >> shift) & dmask);
        if (((key ^ pa) & above) != 0) {
            if (same || ((key ^ pb) & above) != 0) continue;
            bin += kSkyBins;
        }
        if (bin == run_bin) {
            ++run;
        } else {
            if (run) rt::atomic_add_i32(lh + run_bin, run);
            run_bin = bin;
            run = 1;
        }
    }
    if (run) rt::atomic_add_i32(lh + run_bin, run);
    rt::block_sync_lds();
    int32_t* gh = sky_hist(work, nframes, f);
    for (int i = tid; i < 2 * kSkyBins; i += kSkyThreads) {
        const int c = lh[i];
        if (c) rt::atomic_add_i32(gh + i, c);
    }
}

// In hist[0 .. kSkyBins) (thread t owns bins 8 t .. 8 t + 7, `off` = the count below its first bin) the bin that
// holds `rank`: written by the one thread that owns it to res[0] = bin, res[1] = rank inside the bin, res[2] = the
// bin's count.
SPX_DEVICE void sky_find(const int32_t* hist, long long off, long long rank, long long* res) {
    const int t = rt::thread_id();
    long long below = off;
    for (int k = 0; k < 8; ++k) {
        const long long c = hist[8 * t + k];
        if (rank >= below && rank < below + c) {
            res[0] = 8 * t + k;
            res[1] = rank - below;
            res[2] = c;
        }
        below += c;
    }
}

// One workgroup per frame.  pass 0 opens a round: the histogram's total is the count inside the candidate range.
template <typename T>
SPX_TKERNEL(256)
void sky_select_kernel(int nframes, int pass, int round, void* __restrict__ work) {
    SPX_DYN_LDS(lds_raw);
    long long* sums = reinterpret_cast<long long*>(lds_raw);         // [256] per-thread sums, then [8] results
    long long* res = sums + kSkyThreads;
    const int tid = rt::thread_id();
    const int f = (int)rt::block_id();
    if (f >= nframes) return;
    SkyState* st = sky_state(work, f);
    if (st->done) return;
    int32_t* gh = sky_hist(work, nframes, f);
    const bool same = st->same != 0;
    long long own[2] = {0, 0};
    for (int h = 0; h < 2; ++h)
        for (int k = 0; k < 8; ++k) own[h] += gh[h * kSkyBins + 8 * tid + k];
    long long off[2];
    for (int h = 0; h < 2; ++h) {
        sums[tid] = own[h];
        rt::block_sync_lds();
        long long o = 0;
        for (int k = 0; k < tid; ++k) o += sums[k];
        off[h] = o;
        if (h == 0 && tid == kSkyThreads - 1) res[6] = o + own[0];   // the total of histogram 0
        rt::block_sync_lds();
    }
    const long long total = res[6];
    // round logic: every thread takes the same decision from the same numbers
    long long n = st->n;
    if (pass == 0) {
        bool stop = false;
        if (round == 0) {
            if (total == 0) stop = true;
        } else if (total == n || total == 0) {
            stop = true;                                             // step 5: nothing was cut, or all would be
        }
        if (stop) {
            rt::block_sync_lds();
            if (tid == 0) {
                if (round == 0) st->status |= kSkyEmpty;
                st->done = 1;
            }
            for (int k = 0; k < 8; ++k) gh[8 * tid + k] = gh[kSkyBins + 8 * tid + k] = 0;
            return;
        }
        n = total;
    }
    const long long ra = pass == 0 ? (n - 1) / 2 : st->rank[0], rb = pass == 0 ? n / 2 : st->rank[1];
    sky_find(gh, off[0], ra, res);
    sky_find(same ? gh : gh + kSkyBins, same ? off[0] : off[1], rb, res + 3);
    rt::block_sync_lds();
    const int shift = sky_digit_shift(SkyKey<T>::bits, pass);
    const unsigned long long ka = (pass == 0 ? 0ull : st->prefix[0]) | ((unsigned long long)res[0] << shift);
    const unsigned long long kb = (pass == 0 ? 0ull : st->prefix[1]) | ((unsigned long long)res[3] << shift);
    const bool still = same && res[0] == res[3];
    rt::block_sync();                                                // every thread has read the state (global)
    if (tid == 0) {
        if (pass == 0) {
            st->n = n;
            if (round == 0) st->n_usable = n;
            st->lo = st->cand_lo;
            st->hi = st->cand_hi;
            st->rounds = round + 1;
        }
        st->prefix[0] = ka;
        st->prefix[1] = kb;
        st->rank[0] = res[1];
        st->rank[1] = res[4];
        st->same = (pass == SkyKey<T>::digits - 1) ? 1 : (still ? 1 : 0);     // the next round starts on one prefix
        if (pass == SkyKey<T>::digits - 1) {
            const double a = SkyKey<T>::value(ka), c = SkyKey<T>::value(kb);
            st->med = (n & 1) ? a : (a + c) * 0.5;
            if (still && res[2] == n) {                              // one key holds every value: min == max
                st->mean = a;
                st->sd = 0.0;
                st->need_moments = 0;
                st->done = 1;
            } else {
                st->need_moments = 1;
            }
        }
    }
    for (int k = 0; k < 8; ++k) gh[8 * tid + k] = gh[kSkyBins + 8 * tid + k] = 0;
}

// sum over the workgroup in the order of the header: wave butterfly, then the wave sums in wave order
SPX_DEVICE double sky_block_sum(double* red, double v) {
    for (int m = 32; m > 0; m >>= 1) v = v + rt::shfl_xor(v, m);
    const int tid = rt::thread_id();
    rt::block_sync_lds();                                            // red may still be read by the previous call
    if ((tid & 63) == 0) red[tid >> 6] = v;
    rt::block_sync_lds();
    double s = 0.0;
    for (int w = 0; w < kSkyThreads / 64; ++w) s = s + red[w];
    return s;
}

// grid = nframes * kSkyMomentGrid, exactly.
template <typename T>
SPX_TKERNEL(256)
void sky_moments_kernel(const T* const* __restrict__ frames, const T* const* __restrict__ weights,
                        const uint8_t* const* __restrict__ masks, const int32_t* __restrict__ shapes, int nframes,
                        void* __restrict__ work) {
#pragma clang fp contract(off)
    SPX_DYN_LDS(lds_raw);
    double* red = reinterpret_cast<double*>(lds_raw);
    const int tid = rt::thread_id();
    const int f = (int)(rt::block_id() / kSkyMomentGrid), b = (int)(rt::block_id() - (int64_t)f * kSkyMomentGrid);
    if (f >= nframes) return;
    const SkyState* st = sky_state(work, f);
    if (st->done || !st->need_moments) return;
    const long long npix = (long long)shapes[2 * f] * shapes[2 * f + 1];
    const T* frame = frames[f];
    const T* weight = weights ? weights[f] : nullptr;
    const uint8_t* mask = masks ? masks[f] : nullptr;
    const double lo = st->lo, hi = st->hi, med = st->med;
    double s1 = 0.0, s2 = 0.0;
    for (long long i = (long long)b * kSkyThreads + tid; i < npix; i += kSkyStride) {
        T v;
        if (!sky_in_range(frame, weight, mask, i, lo, hi, &v)) continue;
        const double d = (double)v - med;
        s1 = s1 + d;
        s2 = s2 + d * d;
    }
    s1 = sky_block_sum(red, s1);
    s2 = sky_block_sum(red, s2);
    if (tid == 0) {
        double* p = sky_partials(work, nframes, f) + 2 * b;
        p[0] = s1;
        p[1] = s2;
    }
}

// One thread per frame: mean and std of the round, step 4, and the candidate range of step 5.
SPX_TKERNEL(256)
void sky_finish_kernel(int nframes, int round, int max_iters, double lsigma, double usigma, void* __restrict__ work) {
#pragma clang fp contract(off)
    const int f = rt::thread_id();
    if (rt::block_id() != 0 || f >= nframes) return;
    SkyState* st = sky_state(work, f);
    if (st->done || !st->need_moments) return;
    const double* p = sky_partials(work, nframes, f);
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < kSkyMomentGrid; ++b) {
        s1 = s1 + p[2 * b];
        s2 = s2 + p[2 * b + 1];
    }
    const double n = (double)st->n, m1 = s1 / n;
    const double var = s2 / n - m1 * m1;
    const double sd = __builtin_sqrt(var > 0.0 ? var : 0.0);
    st->mean = st->med + m1;
    st->sd = sd;
    st->need_moments = 0;
    if (!(sd > 0.0) || round >= max_iters) {
        st->done = 1;
        return;
    }
    const double a = st->med - lsigma * sd, c = st->med + usigma * sd;
    st->cand_lo = st->lo > a ? st->lo : a;
    st->cand_hi = st->hi < c ? st->hi : c;
}

// One thread per frame.  out [nframes][6] = sky med mean std lo hi, counts [nframes][2], status [nframes][2].
SPX_TKERNEL(256)
void sky_output_kernel(int nframes, int stat, const void* __restrict__ work, double* __restrict__ out,
                       long long* __restrict__ out_counts, int32_t* __restrict__ out_status) {
#pragma clang fp contract(off)
    const int f = rt::thread_id();
    if (rt::block_id() != 0 || f >= nframes) return;
    const SkyState* st = reinterpret_cast<const SkyState*>(work) + f;
    const double med = st->med, mean = st->mean, sd = st->sd;
    double sky = med;
    if (stat == kSkyMean) sky = mean;
    if (stat == kSkyMode) {
        if (sd == 0.0) sky = mean;
        else if (__builtin_fabs(mean - med) < 0.3 * sd) sky = 2.5 * med - 1.5 * mean;
        else sky = med;
    }
    double* o = out + 6 * f;
    o[0] = sky; o[1] = med; o[2] = mean; o[3] = sd; o[4] = st->lo; o[5] = st->hi;
    out_counts[2 * f] = st->n_usable;
    out_counts[2 * f + 1] = st->n;
    out_status[2 * f] = st->status;
    out_status[2 * f + 1] = st->rounds;
}

namespace host {
// The launch sequence, written once: `launch(kind, pass, round)` enqueues one kernel, kind 0 = init, 1 = hist,
// 2 = select, 3 = moments, 4 = finish, 5 = output.
template <typename L> void sky_stats_launch(int digits, int max_iters, L&& launch) {
    launch(0, 0, 0);
    for (int r = 0; r <= max_iters; ++r) {
        for (int p = 0; p < digits; ++p) {
            launch(1, p, r);
            launch(2, p, r);
        }
        launch(3, 0, r);
        launch(4, 0, r);
    }
    launch(5, 0, 0);
}
// frame reads of one call (hist passes and moments passes), COUNTED from the sequence above
constexpr int sky_frame_reads(int digits, int max_iters) { return (max_iters + 1) * (digits + 1); }
}  // namespace host

}  // namespace spx
