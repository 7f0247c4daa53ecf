// TEST INFRASTRUCTURE ONLY: a stand-alone program over emu_minmed.cpp for a sanitizer pass on the CPU (every buffer here
// has exactly the size the C ABI asks for and the LDS block exactly the launch's size, so an address sanitizer reports
// any access beyond them; every work-item is a CPU thread, so a thread sanitizer reports a missing barrier, two threads
// writing one output, or a pass that reads a plane another thread of it writes).  Build and run, from the repository
// root:
//   clang++ -std=c++20 -O1 -g -pthread -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -Isubpixal_amd/csrc -Itests/cpu_emu -o /tmp/emu_minmed_main tests/cpu_emu/emu_minmed_main.cpp
//   /tmp/emu_minmed_main            (or -fsanitize=thread instead)
// Scenes of K = 2, 3 and 5 frames of different shapes in float32 and float64 -- dithered, rotated, one narrower than a
// tile, one inactive -- with noise, drawn hits, a weight map (a zero and a NaN), a NaN pixel, a mask and an rms map with
// a NaN, on a 21 x 45 output (no multiple of the 32 x 8 tile), with combine_grow 0, 1 and 8 (nsigma 1 and 0.5, nhigh 1
// at K = 5, a gain with combine_grow 1) and the growth settings (g, c, ctedir) = (3, 0, 0), (9, 5, +1), (1, 64, -1) and
// (1, 0, 0), once with one workgroup looping over all tiles and once with one workgroup per tile.  It checks the invariants that need no second implementation: md and nmed equal
// to the median kernel's, lo <= md, the plane in {0, 1, 2} and consistent with the bits, med = lo or md by the plane;
// the grown mask contains its seed, grows only onto finite, unmasked pixels of positive weight and valid rms, clean
// is unchanged off the newly flagged pixels and finite on them, (1, 0, 0) changes nothing, both grids bit-identical.
#include "emu_minmed.cpp"

#include <cstdio>

namespace {
struct Spec { int ny, nx; double deg, tx, ty; int active; };

double noise(uint32_t& s) {                       // a cheap symmetric deviate in (-1.5, 1.5)
    double v = 0.0;
    for (int q = 0; q < 3; ++q) {
        s = s * 1664525u + 1013904223u;
        v += (double)(s >> 8) / 16777216.0 - 0.5;
    }
    return v;
}

template <typename T>
int run(int K, int grow, double gain) {
    const int NY = 21, NX = 45;
    const int nhigh = K == 5 ? 1 : 0;
    const std::vector<Spec> all = {{18, 40, 0.0, 2.0, 1.0, 1},  {18, 40, 1.0, 3.3, 1.6, 1}, {33, 9, 3.0, 14.5, -6.0, 1},
                                   {18, 40, -1.5, 2.6, 2.2, 0}, {9, 5, 0.0, 20.25, 6.5, 1}};
    const std::vector<Spec> specs(all.begin(), all.begin() + K);
    std::vector<std::vector<T>> data((size_t)K), wgt((size_t)K), rms((size_t)K);
    std::vector<std::vector<uint8_t>> msk((size_t)K);
    std::vector<const T*> dp, wp;
    std::vector<const uint8_t*> mp;
    std::vector<int32_t> shapes;
    std::vector<double> maps, table;
    std::vector<uint8_t> active;
    uint32_t seed = 2468u;
    for (int k = 0; k < K; ++k) {
        const Spec& s = specs[(size_t)k];
        const size_t n = (size_t)s.ny * s.nx;
        const double th = s.deg * 3.14159265358979323846 / 180.0, c = std::cos(th), sn = std::sin(th);
        const double m[6] = {c, -sn, s.tx, sn, c, s.ty};
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
                if ((i * 7 + j * 13 + k) % 53 == 0) v += 1.0;             // a hit
                const size_t q = (size_t)j * s.nx + i;
                data[(size_t)k][q] = (T)v;
                wgt[(size_t)k][q] = (T)(0.5 + 0.01 * (double)(q % 13));
            }
        data[(size_t)k][n / 2] = (T)__builtin_nan("");
        wgt[(size_t)k][1] = (T)0;
        wgt[(size_t)k][3] = (T)__builtin_nan("");
        msk[(size_t)k][n - 1] = 1;
        msk[(size_t)k][n / 4] = 1;
        rms[(size_t)k][n / 3] = (T)__builtin_nan("");
        dp.push_back(data[(size_t)k].data());
        wp.push_back(k == 1 ? nullptr : wgt[(size_t)k].data());
        mp.push_back(k == 2 ? nullptr : msk[(size_t)k].data());
        shapes.push_back(s.ny);
        shapes.push_back(s.nx);
        active.push_back((uint8_t)s.active);
        table.insert(table.end(), {0.05 + 0.01 * k, 0.2, gain});
    }
    int bad = 0;
    const size_t npix = (size_t)NY * NX;
    std::vector<float> med0(npix, -77.0f);
    std::vector<uint8_t> nmed0(npix, 201);
    if (crr_median<T>(dp.data(), wp.data(), mp.data(), shapes.data(), maps.data(), active.data(), K, 1.0, 0, 0, nhigh, NY,
                      NX, med0.data(), nmed0.data(), 0))
        return 1;
    std::vector<float> md[2], lo[2], med[2];
    std::vector<uint8_t> bits[2], nmed[2], how[2];
    for (int g = 0; g < 2; ++g) {
        md[g].assign(npix, -77.0f);
        lo[g].assign(npix, -77.0f);
        med[g].assign(npix, -77.0f);
        bits[g].assign(npix, 201);
        nmed[g].assign(npix, 201);
        how[g].assign(npix, 201);
        if (mm_minmed<T>(dp.data(), wp.data(), mp.data(), shapes.data(), maps.data(), active.data(), K, 1.0, 0, 0, nhigh,
                         table.data(), 1.0, 0.5, grow, NY, NX, md[g].data(), lo[g].data(), bits[g].data(), med[g].data(),
                         nmed[g].data(), how[g].data(), g ? 0 : 1))
            return 1;
    }
    if (std::memcmp(md[0].data(), md[1].data(), npix * 4) || std::memcmp(lo[0].data(), lo[1].data(), npix * 4) ||
        std::memcmp(med[0].data(), med[1].data(), npix * 4) || std::memcmp(bits[0].data(), bits[1].data(), npix) ||
        std::memcmp(nmed[0].data(), nmed[1].data(), npix) || std::memcmp(how[0].data(), how[1].data(), npix))
        ++bad;
    if (std::memcmp(md[0].data(), med0.data(), npix * 4) || std::memcmp(nmed[0].data(), nmed0.data(), npix)) ++bad;
    size_t by_own = 0, by_rule = 0;
    for (size_t q = 0; q < npix; ++q) {
        const int b = bits[0][q], h = how[0][q];
        if (b > 3 || b == 1 || h > 2) ++bad;                      // hit_1 implies hit_2
        if ((h == 1) != ((b & 1) != 0)) ++bad;
        if (h == 2 && (b != 2 || grow == 0)) ++bad;
        if (nmed[0][q] < 2 && b) ++bad;
        if (nmed[0][q] && !(lo[0][q] <= md[0][q])) ++bad;
        const float want = h ? lo[0][q] : md[0][q];
        if (std::memcmp(&med[0][q], &want, 4)) ++bad;
        by_own += h == 1;
        by_rule += h == 2;
    }
    if (by_own == 0) ++bad;
    // the comparison and the growth, on the minmed image
    const int settings[4][3] = {{3, 0, 0}, {9, 5, 1}, {1, 64, -1}, {1, 0, 0}};
    size_t grown_px = 0;
    for (int k = 0; k < K; ++k) {
        if (!specs[(size_t)k].active) continue;
        const size_t n = data[(size_t)k].size();
        const T* rmap = k % 2 ? nullptr : rms[(size_t)k].data();
        std::vector<uint8_t> sd(n, 201);
        std::vector<T> cl(n, (T)-77);
        if (crr_cr<T>(dp.data(), wp.data(), mp.data(), shapes.data(), maps.data(), active.data(), K, 1.0, 0, k,
                      med[0].data(), nmed[0].data(), NY, NX, 0.05, rmap, 0.2, gain, 3.5, 3.0, 1.2, 0.7, sd.data(),
                      cl.data(), 0))
            return 1;
        for (const auto& st : settings) {
            std::vector<uint8_t> gm[2];
            std::vector<T> gc[2];
            for (int g = 0; g < 2; ++g) {
                gm[g].assign(n, 201);
                gc[g] = cl;
                if (mm_cr_grow<T>(dp.data(), wp.data(), mp.data(), shapes.data(), maps.data(), active.data(), K, 1.0, 0, k,
                                  med[0].data(), nmed[0].data(), NY, NX, 0.05, rmap, sd.data(), st[0], st[1], st[2],
                                  gm[g].data(), gc[g].data(), g ? 0 : 1))
                    return 1;
            }
            if (std::memcmp(gm[0].data(), gm[1].data(), n) || std::memcmp(gc[0].data(), gc[1].data(), n * sizeof(T))) ++bad;
            for (size_t q = 0; q < n; ++q) {
                const T d = data[(size_t)k][q];
                const bool ok = (d - d == T(0)) && !(mp[(size_t)k] && mp[(size_t)k][q]) &&
                                (!wp[(size_t)k] || (wp[(size_t)k][q] - wp[(size_t)k][q] == T(0) && wp[(size_t)k][q] > T(0))) &&
                                (!rmap || rmap[q] - rmap[q] == T(0));
                const bool fresh = gm[0][q] && !sd[q];
                if (gm[0][q] > 1 || (sd[q] && !gm[0][q]) || (fresh && !ok)) ++bad;
                if (fresh) {
                    ++grown_px;
                    if (!(gc[0][q] - gc[0][q] == T(0))) ++bad;
                } else if (std::memcmp(&gc[0][q], &cl[q], sizeof(T))) {
                    ++bad;
                }
                if (st[0] == 1 && st[1] == 0 && fresh) ++bad;
            }
        }
    }
    std::printf("K %d grow %d gain %.0f (%s): %zu pixels take the minimum by their own test, %zu by the neighbour rule, "
                "%zu pixels newly flagged by the growth\n", K, grow, gain, sizeof(T) == 8 ? "float64" : "float32", by_own,
                by_rule, grown_px);
    if (grown_px == 0) ++bad;
    return bad;
}
}  // namespace

int main() {
    int bad = 0;
    for (int K : {2, 3, 5})
        for (int grow : {0, 1, 8}) {
            const double gain = grow == 1 ? 2000.0 : 0.0;
            bad += run<float>(K, grow, gain) + run<double>(K, grow, gain);
        }
    std::printf(bad ? "FAILED\n" : "OK\n");
    return bad ? 1 : 0;
}
