// TEST INFRASTRUCTURE ONLY: a stand-alone program over a few cases of the whole-frame statistics harness
// (emu_sky.cpp), for sanitizer builds:
//   clang++ -std=c++20 -O1 -g -pthread -fsanitize=address,undefined -Isubpixal_amd/csrc -Itests/cpu_emu
//           tests/cpu_emu/emu_sky_main.cpp -o emu_sky_asan        (and -fsanitize=thread)
// It checks the results against a sort on the host, so it also fails on a wrong answer.
#include "emu_sky.cpp"

#include <algorithm>
#include <cstdio>

namespace {
unsigned long long g_seed = 88172645463325252ull;
double uniform() {
    g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17;
    return (double)(g_seed >> 11) / 9007199254740992.0;
}

template <typename T> int run_case(const char* name, int ny, int nx, int kind) {
    std::vector<T> a((size_t)ny * nx), w((size_t)ny * nx, T(1));
    std::vector<uint8_t> m((size_t)ny * nx, 0);
    for (size_t i = 0; i < a.size(); ++i) {
        double v = 100.0 + 3.0 * (uniform() + uniform() + uniform() - 1.5);
        if (kind == 1) v = 7.25;                                   // constant
        if (kind == 2) v = (i & 1) ? 1.0 : 2.0;                    // two values
        if (kind == 3 && i % 17 == 0) v = 5000.0 * uniform();      // bright sources
        a[i] = (T)v;
        if (kind == 3 && i % 29 == 0) a[i] = (T)__builtin_nan("");
        if (kind == 3 && i % 31 == 0) m[i] = 1;
        if (kind == 3 && i % 37 == 0) w[i] = T(0);
    }
    // the same frame twice in a batch, and a one-pixel frame between them
    T one = T(-0.0);
    const void* frames[3] = {a.data(), &one, a.data()};
    const void* weights[3] = {w.data(), nullptr, w.data()};
    const uint8_t* masks[3] = {m.data(), nullptr, m.data()};
    const int32_t shapes[6] = {ny, nx, 1, 1, ny, nx};
    double out[18];
    long long counts[6];
    int32_t status[6];
    const double nan = __builtin_nan("");
    int rc = sizeof(T) == 4
        ? emus_sky_stats_f32(frames, weights, masks, shapes, 3, nan, nan, 3.0, 2.5, 3, kSkyMode, out, counts, status, 3)
        : emus_sky_stats_f64(frames, weights, masks, shapes, 3, nan, nan, 3.0, 2.5, 3, kSkyMode, out, counts, status, 3);
    if (rc) return 1;
    // round 0 by sorting
    std::vector<double> u;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i] - a[i] == T(0) && !m[i] && w[i] > T(0)) u.push_back((double)a[i]);
    std::sort(u.begin(), u.end());
    int bad = 0;
    if (counts[0] != (long long)u.size() || counts[4] != counts[0] || counts[2] != 1) bad |= 1;
    if (std::memcmp(out, out + 12, 6 * sizeof(double)) != 0) bad |= 2;            // batch position does not matter
    if (!(out[7] == 0.0 && out[9] == 0.0 && status[3] == 1)) bad |= 4;            // the one-pixel frame
    if (kind == 1 && !(out[1] == 7.25 && out[3] == 0.0 && status[1] == 1)) bad |= 8;
    if (kind == 2 && !(out[1] == 1.5)) bad |= 16;
    if (!(out[4] <= out[1] && out[1] <= out[5])) bad |= 32;
    std::printf("%-22s %s n_usable %lld n_final %lld rounds %d med %.9g mean %.9g std %.9g -> %s\n", name,
                sizeof(T) == 4 ? "f32" : "f64", counts[0], counts[1], status[1], out[1], out[2], out[3],
                bad ? "FAILED" : "ok");
    return bad;
}
}  // namespace

int main() {
    int bad = 0;
    bad |= run_case<float>("noise 67x45", 67, 45, 0);
    bad |= run_case<double>("noise 67x45", 67, 45, 0);
    bad |= run_case<float>("constant 33x21", 33, 21, 1);
    bad |= run_case<double>("two values 8x7", 8, 7, 2);
    bad |= run_case<float>("sources, nan, mask 101x61", 101, 61, 3);
    bad |= run_case<double>("sources, nan, mask 101x61", 101, 61, 3);
    std::printf(bad ? "FAILED (%d)\n" : "all ok\n", bad);
    return bad ? 1 : 0;
}
