// TEST INFRASTRUCTURE ONLY: a stand-alone program over emu_crreject.cpp for a sanitizer pass on the CPU (every buffer
// here has exactly the size the C ABI asks for and the LDS block exactly the launch's size, so an address sanitizer
// reports any access beyond them; every work-item is a CPU thread, so a thread sanitizer reports a missing barrier
// or two threads writing one output).  Build and run, from the repository root:
//   clang++ -std=c++20 -O1 -g -pthread -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -Isubpixal_amd/csrc -Itests/cpu_emu -o /tmp/emu_crreject_main tests/cpu_emu/emu_crreject_main.cpp
//   /tmp/emu_crreject_main            (or -fsanitize=thread instead)
// Six frames of different shapes in float32 and float64 -- dithered, rotated, mirrored, half outside the output,
// narrower than a tile, one inactive -- with noise, drawn hits, weights (a zero and a NaN), a NaN pixel, a mask and an
// rms map with a NaN, on a 21 x 45 output (no multiple of the 32 x 8 tile), for 'square' and 'turbo', pixfrac 1 and
// 0.5, nhigh 0 and 1, once with one workgroup looping over all tiles and once with one workgroup per tile.  It
// checks the invariants that need no second implementation: nmed <= the number of active frames, med within the
// range of the frames' values where nmed > 0 and 0 elsewhere, crmask in {0, 1} and only on pixels that are finite,
// unmasked, of positive weight and of valid rms, clean equal to the frame off the mask and finite on it, hits
// flagged at all, both grids bit-identical.
#include "emu_crreject.cpp"

#include <cstdio>

namespace {
struct Spec { int ny, nx; double deg, tx, ty; bool mirror; int active; };

double noise(uint32_t& s) {                       // a cheap symmetric deviate in (-1.5, 1.5)
    double v = 0.0;
    for (int q = 0; q < 3; ++q) {
        s = s * 1664525u + 1013904223u;
        v += (double)(s >> 8) / 16777216.0 - 0.5;
    }
    return v;
}

template <typename T>
int run(int kernel, double pixfrac, int nhigh) {
    const int NY = 21, NX = 45;
    const std::vector<Spec> specs = {{18, 40, 0.0, 2.0, 1.0, false, 1},  {18, 40, 1.0, 3.3, 1.6, false, 1},
                                     {18, 40, -1.5, 2.6, 2.2, false, 1}, {20, 25, 30.0, 12.5, 3.0, true, 0},
                                     {33, 9, 3.0, -4.5, -12.0, false, 1}, {9, 5, 0.0, 20.25, 6.5, false, 1}};
    const int K = (int)specs.size();
    std::vector<std::vector<T>> data((size_t)K), wgt((size_t)K), rms((size_t)K);
    std::vector<std::vector<uint8_t>> msk((size_t)K);
    std::vector<const T*> dp, wp;
    std::vector<const uint8_t*> mp;
    std::vector<int32_t> shapes;
    std::vector<double> maps;
    std::vector<uint8_t> active;
    double lo = 1e300, hi = -1e300;
    uint32_t seed = 12345u;
    int nactive = 0;
    for (int k = 0; k < K; ++k) {
        const Spec& s = specs[(size_t)k];
        const size_t n = (size_t)s.ny * s.nx;
        const double th = s.deg * 3.14159265358979323846 / 180.0, c = std::cos(th), sn = std::sin(th);
        const double sx = s.mirror ? -1.0 : 1.0;
        const double m[6] = {c * sx, -sn, s.tx + (s.mirror ? 0.8 * s.nx : 0.0), sn * sx, c, s.ty};
        maps.insert(maps.end(), m, m + 6);
        data[(size_t)k].resize(n);
        wgt[(size_t)k].resize(n);
        rms[(size_t)k].assign(n, (T)0.05);
        msk[(size_t)k].assign(n, 0);
        for (int j = 0; j < s.ny; ++j)
            for (int i = 0; i < s.nx; ++i) {
                const double X = m[0] * i + m[1] * j + m[2], Y = m[3] * i + m[4] * j + m[5];
                double v = 1.0 + 0.01 * X + 2.0 * std::exp(-((X - 20.0) * (X - 20.0) + (Y - 9.0) * (Y - 9.0)) / 12.5);
                v += 0.05 * noise(seed);
                if ((i * 7 + j * 13 + k) % 97 == 0) v += 1.0;             // a hit
                const size_t q = (size_t)j * s.nx + i;
                data[(size_t)k][q] = (T)v;
                wgt[(size_t)k][q] = (T)(0.5 + 0.01 * (double)(q % 13));
                lo = std::fmin(lo, (double)(T)v);
                hi = std::fmax(hi, (double)(T)v);
            }
        data[(size_t)k][n / 2] = (T)__builtin_nan("");
        wgt[(size_t)k][1] = (T)0;
        wgt[(size_t)k][3] = (T)__builtin_nan("");
        msk[(size_t)k][n - 1] = 1;
        rms[(size_t)k][n / 3] = (T)__builtin_nan("");
        dp.push_back(data[(size_t)k].data());
        wp.push_back(k == 1 ? nullptr : wgt[(size_t)k].data());
        mp.push_back(k == 2 ? nullptr : msk[(size_t)k].data());
        shapes.push_back(s.ny);
        shapes.push_back(s.nx);
        active.push_back((uint8_t)s.active);
        nactive += s.active;
    }
    int bad = 0;
    const size_t npix = (size_t)NY * NX;
    std::vector<float> med[2];
    std::vector<uint8_t> nmed[2];
    for (int g = 0; g < 2; ++g) {
        med[g].assign(npix, -77.0f);
        nmed[g].assign(npix, 201);
        if (crr_median<T>(dp.data(), wp.data(), mp.data(), shapes.data(), maps.data(), active.data(), K, pixfrac, kernel,
                          0, nhigh, NY, NX, med[g].data(), nmed[g].data(), g ? 0 : 1))
            return 1;
    }
    if (std::memcmp(med[0].data(), med[1].data(), npix * 4) || std::memcmp(nmed[0].data(), nmed[1].data(), npix)) ++bad;
    size_t covered = 0;
    for (size_t q = 0; q < npix; ++q) {
        const double v = med[0][q];
        if (nmed[0][q] > nactive) ++bad;
        if (nmed[0][q]) {
            ++covered;
            if (!(v >= lo - 1e-6 && v <= hi + 1e-6)) ++bad;
        } else if (v != 0.0) {
            ++bad;
        }
    }
    if (covered == 0 || covered == npix) ++bad;
    size_t flagged = 0;
    for (int k = 0; k < K; ++k) {
        if (!specs[(size_t)k].active) continue;
        const size_t n = data[(size_t)k].size();
        std::vector<uint8_t> crm[2];
        std::vector<T> cln[2];
        const T* rmap = k % 2 ? nullptr : rms[(size_t)k].data();
        for (int g = 0; g < 2; ++g) {
            crm[g].assign(n, 201);
            cln[g].assign(n, (T)-77);
            if (crr_cr<T>(dp.data(), wp.data(), mp.data(), shapes.data(), maps.data(), active.data(), K, pixfrac, kernel,
                          k, med[0].data(), nmed[0].data(), NY, NX, 0.05, rmap, 0.2, k == 2 ? 50.0 : -1.0, 3.5, 3.0,
                          1.2, 0.7, crm[g].data(), cln[g].data(), g ? 0 : 1))
                return 1;
        }
        if (std::memcmp(crm[0].data(), crm[1].data(), n) || std::memcmp(cln[0].data(), cln[1].data(), n * sizeof(T))) ++bad;
        for (size_t q = 0; q < n; ++q) {
            const T d = data[(size_t)k][q];
            const bool ok = (d - d == T(0)) && !(mp[(size_t)k] && mp[(size_t)k][q]) &&
                            (!wp[(size_t)k] || (wp[(size_t)k][q] - wp[(size_t)k][q] == T(0) && wp[(size_t)k][q] > T(0))) &&
                            (!rmap || rmap[q] - rmap[q] == T(0));
            if (crm[0][q] > 1 || (crm[0][q] && !ok)) ++bad;
            if (crm[0][q]) {
                ++flagged;
                if (!(cln[0][q] - cln[0][q] == T(0))) ++bad;
            } else if (std::memcmp(&cln[0][q], &d, sizeof(T))) {
                ++bad;
            }
        }
    }
    std::printf("kernel %d pixfrac %.1f nhigh %d (%s): %zu of %zu output pixels covered, %zu pixels flagged\n", kernel,
                pixfrac, nhigh, sizeof(T) == 8 ? "float64" : "float32", covered, npix, flagged);
    if (flagged == 0) ++bad;
    return bad;
}
}  // namespace

int main() {
    int bad = 0;
    for (int kernel = 0; kernel < 2; ++kernel)
        for (double p : {1.0, 0.5})
            for (int nhigh = 0; nhigh < 2; ++nhigh) bad += run<float>(kernel, p, nhigh) + run<double>(kernel, p, nhigh);
    std::printf(bad ? "FAILED\n" : "OK\n");
    return bad ? 1 : 0;
}
