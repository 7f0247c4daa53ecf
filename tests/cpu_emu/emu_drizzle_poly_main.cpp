// TEST INFRASTRUCTURE ONLY: a stand-alone program over emu_drizzle_poly.cpp for a sanitizer pass on the CPU (every
// buffer here has exactly the size the C ABI asks for, so an address sanitizer reports any access beyond them; every
// work-item is a CPU thread, so a thread sanitizer reports two of them writing one output).  Build and run, from the
// repository root:
//   clang++ -std=c++20 -O1 -g -pthread -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -Isubpixal_amd/csrc -Itests/cpu_emu -o /tmp/emu_drizzle_poly_main tests/cpu_emu/emu_drizzle_poly_main.cpp
//   /tmp/emu_drizzle_poly_main       (or -fsanitize=thread instead)
// Five frames of different shapes in float32 and float64 -- degrees 1, 2, 3 and 5, one mirrored, one shrunk, one that
// misses the output, one inactive, one given about a far centre -- with weights (a zero, a negative and a NaN), a NaN
// pixel and a mask, on a 37 x 70 output (no multiple of the 32 x 8 tile), for the three kernels and pixfrac 1 and
// 0.4, once with one workgroup looping over all tiles and once with one workgroup per tile.  It checks the
// invariants that need no second implementation: wht >= 0 and finite, sci finite and within the data's range where
// wht > 0 and fill elsewhere, ctx zero exactly where wht is zero, no bit of an inactive or absent frame, both grids
// bit-identical; and that the packing refuses what it must.
#include "emu_drizzle_poly.cpp"

#include <cstdio>

namespace {
struct Spec { int ny, nx, degree; double deg, scale, tx, ty, k, q, cx, cy; bool mirror; int active; };

void fill_map(const Spec& s, double* coef, double* center) {
    for (int q = 0; q < 2 * kDrzPolyTerms; ++q) coef[q] = 0.0;
    // about the frame's centre: rotation o (scale (1 + k r^2) (u, v) + q u v), then moved to (cx, cy) by hand for
    // degree <= 2 only (the far centre is used with a degree-1 frame, where the shift is exact to write down)
    const double th = s.deg * 3.14159265358979323846 / 180.0, c = std::cos(th), sn = std::sin(th);
    double f[2][kDrzPolyTerms] = {};
    f[0][drzp_slot(1, 0)] = s.mirror ? -s.scale : s.scale;
    f[1][drzp_slot(0, 1)] = s.scale;
    if (s.degree >= 3) {
        f[0][drzp_slot(3, 0)] = f[0][drzp_slot(1, 2)] = (s.mirror ? -1.0 : 1.0) * s.scale * s.k;
        f[1][drzp_slot(2, 1)] = f[1][drzp_slot(0, 3)] = s.scale * s.k;
    }
    if (s.degree >= 2) {
        f[0][drzp_slot(1, 1)] = s.q;
        f[1][drzp_slot(1, 1)] = -0.5 * s.q;
    }
    if (s.degree >= 5) f[0][drzp_slot(2, 3)] = f[1][drzp_slot(5, 0)] = 1e-9;
    for (int k = 0; k < kDrzPolyTerms; ++k) {
        coef[k] = c * f[0][k] - sn * f[1][k];
        coef[kDrzPolyTerms + k] = sn * f[0][k] + c * f[1][k];
    }
    const double xf = 0.5 * (s.nx - 1), yf = 0.5 * (s.ny - 1);
    center[0] = xf;
    center[1] = yf;
    coef[0] = s.tx;
    coef[kDrzPolyTerms] = s.ty;
    if (s.degree == 1 && (s.cx != 0.0 || s.cy != 0.0)) {      // the same affine about (cx, cy)
        center[0] = s.cx;
        center[1] = s.cy;
        coef[0] += coef[1] * (s.cx - xf) + coef[2] * (s.cy - yf);
        coef[kDrzPolyTerms] += coef[kDrzPolyTerms + 1] * (s.cx - xf) + coef[kDrzPolyTerms + 2] * (s.cy - yf);
    }
}

template <typename T>
int run(int kernel, double pixfrac) {
    const int NY = 37, NX = 70;
    const std::vector<Spec> specs = {
        {40, 48, 3, 20.0, 0.95, 30.0, 18.0, 5.1e-5, 6e-4, 0, 0, false, 1},
        {24, 31, 1, 30.0, 1.2, 48.5, 6.0, 0, 0, 2000.0, -1500.0, true, 1},
        {33, 29, 5, -15.0, 0.45, 20.0, 25.0, 3e-5, 2e-4, 0, 0, false, 1},
        {5, 7, 2, 0.0, 1.0, 500.0, 3.0, 0, 1e-3, 0, 0, false, 1},
        {8, 8, 2, 10.0, 2.0, 20.0, 20.0, 0, 1e-3, 0, 0, false, 0}};
    const int K = (int)specs.size();
    std::vector<std::vector<T>> data((size_t)K), wgt((size_t)K);
    std::vector<std::vector<uint8_t>> msk((size_t)K);
    std::vector<const T*> dp, wp;
    std::vector<const uint8_t*> mp;
    std::vector<int32_t> shapes, degree;
    std::vector<double> coef((size_t)K * 2 * kDrzPolyTerms), center((size_t)K * 2);
    std::vector<uint8_t> active;
    double lo = 1e300, hi = -1e300;
    for (int k = 0; k < K; ++k) {
        const Spec& s = specs[(size_t)k];
        const size_t n = (size_t)s.ny * s.nx;
        data[(size_t)k].resize(n);
        wgt[(size_t)k].resize(n);
        msk[(size_t)k].assign(n, 0);
        for (size_t q = 0; q < n; ++q) {
            const double v = 1.0 + std::sin(0.7 * (double)q + k);
            data[(size_t)k][q] = (T)v;
            wgt[(size_t)k][q] = (T)(0.5 + 0.01 * (double)(q % 13));
            lo = std::fmin(lo, (double)(T)v);
            hi = std::fmax(hi, (double)(T)v);
        }
        data[(size_t)k][n / 2] = (T)__builtin_nan("");
        wgt[(size_t)k][1] = (T)0;
        wgt[(size_t)k][2] = (T)-1;
        wgt[(size_t)k][3] = (T)__builtin_nan("");
        msk[(size_t)k][n - 1] = 1;
        dp.push_back(data[(size_t)k].data());
        wp.push_back(k == 1 ? nullptr : wgt[(size_t)k].data());
        mp.push_back(k == 2 ? nullptr : msk[(size_t)k].data());
        shapes.push_back(s.ny);
        shapes.push_back(s.nx);
        degree.push_back(s.degree);
        fill_map(s, &coef[(size_t)k * 2 * kDrzPolyTerms], &center[(size_t)k * 2]);
        active.push_back((uint8_t)s.active);
    }
    int bad = 0;
    const size_t npix = (size_t)NY * NX;
    std::vector<T> sci[2];
    std::vector<float> wht[2];
    std::vector<int32_t> ctx[2];
    for (int g = 0; g < 2; ++g) {
        sci[g].assign(npix, (T)-77);
        wht[g].assign(npix, -77.0f);
        ctx[g].assign(npix, -77);
        if (const int rc = drizzle_poly<T>(dp.data(), wp.data(), mp.data(), shapes.data(), coef.data(), degree.data(),
                                           center.data(), active.data(), K, pixfrac, kernel, -5.0, NY, NX,
                                           sci[g].data(), wht[g].data(), ctx[g].data(), g ? 0 : 1)) {
            std::printf("the packing refused a frame: %d\n", rc);
            return 1;
        }
    }
    if (std::memcmp(sci[0].data(), sci[1].data(), npix * sizeof(T)) || std::memcmp(wht[0].data(), wht[1].data(), npix * 4) ||
        std::memcmp(ctx[0].data(), ctx[1].data(), npix * 4))
        ++bad;
    double total = 0.0;
    size_t covered = 0;
    for (size_t q = 0; q < npix; ++q) {
        const double w = wht[0][q], s = (double)sci[0][q];
        if (!(w >= 0.0) || !(w - w == 0.0) || !(s - s == 0.0)) ++bad;
        if (w > 0.0) {
            ++covered;
            if (s < lo - 1e-6 || s > hi + 1e-6 || ctx[0][q] == 0) ++bad;
        } else if (s != -5.0 || ctx[0][q] != 0) {
            ++bad;
        }
        if (ctx[0][q] & ~0x7) ++bad;                     // frame 3 misses the output, frame 4 is inactive
        total += w;
    }
    std::printf("kernel %d pixfrac %.1f (%s): %zu of %zu pixels covered, sum wht %.6f\n", kernel, pixfrac,
                sizeof(T) == 8 ? "float64" : "float32", covered, npix, total);
    if (covered == 0 || covered == npix) ++bad;
    return bad;
}

// the packing refuses what it must, and writes a row only for what it accepts
int refusals() {
    DrizzlePolyRow r;
    const double c0[2] = {1.5, 1.5};
    double ok[42] = {}, sing[42] = {}, nan[42] = {}, tiny[42] = {}, fold[42] = {};
    ok[1] = ok[21 + 2] = 1.0;
    sing[1] = 1.0; sing[2] = 2.0; sing[21 + 1] = 2.0; sing[21 + 2] = 4.0;
    nan[1] = nan[21 + 2] = 1.0; nan[0] = __builtin_nan("");
    tiny[1] = tiny[21 + 2] = 0.1;
    fold[1] = fold[21 + 2] = 1.0; fold[drzp_slot(2, 0)] = -0.5;
    int bad = 0;
    bad += host::drizzle_poly_pack_row(&r, nullptr, nullptr, 4, 4, 1, ok, 1, c0, 1.0, 0, &r) != 0;
    bad += host::drizzle_poly_pack_row(&r, nullptr, nullptr, 4, 4, 1, ok, 0, c0, 1.0, 0, &r) != 4;
    bad += host::drizzle_poly_pack_row(&r, nullptr, nullptr, 4, 4, 1, ok, 6, c0, 1.0, 0, &r) != 4;
    bad += host::drizzle_poly_pack_row(&r, nullptr, nullptr, 4, 4, 1, sing, 1, c0, 1.0, 0, &r) != 2;
    bad += host::drizzle_poly_pack_row(&r, nullptr, nullptr, 4, 4, 1, nan, 1, c0, 1.0, 0, &r) != 1;
    bad += host::drizzle_poly_pack_row(&r, nullptr, nullptr, 4, 4, 1, tiny, 1, c0, 1.0, 0, &r) != 3;
    bad += host::drizzle_poly_pack_row(&r, nullptr, nullptr, 4, 4, 1, fold, 2, c0, 1.0, 0, &r) != 2;
    return bad;
}
}  // namespace

int main() {
    int bad = refusals();
    if (bad) std::printf("refusals: %d wrong\n", bad);
    for (int kernel = 0; kernel < 3; ++kernel)
        for (double p : {1.0, 0.4}) bad += run<float>(kernel, p) + run<double>(kernel, p);
    std::printf(bad ? "FAILED\n" : "OK\n");
    return bad ? 1 : 0;
}
