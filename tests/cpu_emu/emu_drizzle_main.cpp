// TEST INFRASTRUCTURE ONLY: a stand-alone program over emu_drizzle.cpp for a sanitizer pass on the CPU (every buffer
// here has exactly the size the C ABI asks for, so an address sanitizer reports any access beyond them; every
// work-item is a CPU thread, so a thread sanitizer reports two of them writing one output).  Build and run, from the
// repository root:
//   clang++ -std=c++20 -O1 -g -pthread -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -Isubpixal_amd/csrc -Itests/cpu_emu -o /tmp/emu_drizzle_main tests/cpu_emu/emu_drizzle_main.cpp
//   /tmp/emu_drizzle_main            (or -fsanitize=thread instead)
// Five frames of different shapes in float32 and float64 -- rotated, mirrored, shrunk, half outside the output, one
// that misses it, one inactive -- with weights (a zero, a negative and a NaN), a NaN pixel and a mask, on a 37 x 53
// output (no multiple of the 32 x 8 tile), for the three kernels and pixfrac 1 and 0.4, once with one workgroup
// looping over all tiles and once with one workgroup per tile.  It checks the invariants that need no second
// implementation: wht >= 0 and finite, sci finite and within the data's range where wht > 0 and fill elsewhere,
// ctx zero exactly where wht is zero, no bit of an inactive or absent frame, both grids bit-identical.
#include "emu_drizzle.cpp"

#include <cstdio>

namespace {
struct Spec { int ny, nx; double deg, scale, tx, ty; bool mirror; int active; };

template <typename T>
int run(int kernel, double pixfrac) {
    const int NY = 37, NX = 53;
    const std::vector<Spec> specs = {{24, 31, 0.3, 1.0, 3.2, 4.1, false, 1},   {20, 25, 30.0, 1.2, 18.5, -6.0, true, 1},
                                     {13, 9, 77.0, 0.45, 40.0, 20.0, false, 1}, {5, 7, 0.0, 1.0, 500.0, 3.0, false, 1},
                                     {8, 8, 10.0, 2.0, 20.0, 20.0, false, 0}};
    const int K = (int)specs.size();
    std::vector<std::vector<T>> data((size_t)K), wgt((size_t)K);
    std::vector<std::vector<uint8_t>> msk((size_t)K);
    std::vector<const T*> dp, wp;
    std::vector<const uint8_t*> mp;
    std::vector<int32_t> shapes;
    std::vector<double> maps;
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
        const double th = s.deg * 3.14159265358979323846 / 180.0, c = s.scale * std::cos(th), sn = s.scale * std::sin(th);
        const double sx = s.mirror ? -1.0 : 1.0;
        maps.insert(maps.end(), {c * sx, -sn, s.tx + (s.mirror ? 0.8 * s.nx : 0.0), sn * sx, c, s.ty});
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
        if (drizzle<T>(dp.data(), wp.data(), mp.data(), shapes.data(), maps.data(), active.data(), K, pixfrac, kernel,
                       -5.0, NY, NX, sci[g].data(), wht[g].data(), ctx[g].data(), g ? 0 : 1))
            return 1;
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
    DrizzleRow r;
    const double ok[6] = {1, 0, 0, 0, 1, 0}, sing[6] = {1, 2, 0, 2, 4, 0}, nan[6] = {1, 0, __builtin_nan(""), 0, 1, 0},
                 tiny[6] = {0.1, 0, 0, 0, 0.1, 0};
    int bad = 0;
    bad += host::drizzle_pack_row(&r, nullptr, nullptr, 4, 4, 1, ok, 1.0, 0, &r) != 0;
    bad += host::drizzle_pack_row(&r, nullptr, nullptr, 4, 4, 1, sing, 1.0, 0, &r) != 2;
    bad += host::drizzle_pack_row(&r, nullptr, nullptr, 4, 4, 1, nan, 1.0, 0, &r) != 1;
    bad += host::drizzle_pack_row(&r, nullptr, nullptr, 4, 4, 1, tiny, 1.0, 0, &r) != 3;
    return bad;
}
}  // namespace

int main() {
    int bad = refusals();
    for (int kernel = 0; kernel < 3; ++kernel)
        for (double p : {1.0, 0.4}) bad += run<float>(kernel, p) + run<double>(kernel, p);
    std::printf(bad ? "FAILED\n" : "OK\n");
    return bad ? 1 : 0;
}
