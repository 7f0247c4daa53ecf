// TEST INFRASTRUCTURE ONLY: a stand-alone program over emu_errors.cpp for a sanitizer pass on the CPU (the harness
// allocates LDS with exactly the size of the real launch, and every buffer here has exactly the size the C ABI
// asks for, so an address sanitizer reports any access beyond them).  Build and run, from the repository root:
//   clang++ -std=c++20 -O1 -g -pthread -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -Isubpixal_amd/csrc -Itests/cpu_emu -o /tmp/emu_errors_main tests/cpu_emu/emu_errors_main.cpp
//   /tmp/emu_errors_main             (or -fsanitize=thread instead)
// Two scenes in float32 and float64: stars of several sizes (one on the frame's corner, one box above 256 px)
// with an rms map that holds a zero, a negative and a NaN pixel, and a 1 x 1 frame.  Boxes and the measure table
// come from the emulated spx_label_bboxes_i32 / spx_measure_labels_*.  It prints fluxerr and fwhm per source and
// checks the invariants that need no second implementation.
#include "emu_errors.cpp"

#include <cstdio>

namespace {
struct Star { double y, x, amp, sigma; };

template <typename T>
int run(const char* what, int ny, int nx, const std::vector<Star>& stars, double thr, bool bad_rms, int expect) {
    std::vector<T> frame((size_t)ny * nx), rms((size_t)ny * nx);
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            double v = 0.03 * std::sin(1.7 * x + 0.9 * y);
            for (const Star& s : stars)
                v += s.amp * std::exp(-((y - s.y) * (y - s.y) + (x - s.x) * (x - s.x)) / (2.0 * s.sigma * s.sigma));
            frame[(size_t)y * nx + x] = (T)v;
            rms[(size_t)y * nx + x] = (T)(0.05 + 0.001 * (x % 7));
        }
    // labels 1..n in raster order of the first pixel, 8-connected
    std::vector<int32_t> labels((size_t)ny * nx, 0);
    int n = 0;
    std::vector<int> stack;
    for (int p = 0; p < ny * nx; ++p) {
        if (labels[p] || !((double)frame[p] > thr)) continue;
        labels[p] = ++n;
        stack.push_back(p);
        while (!stack.empty()) {
            const int q = stack.back();
            stack.pop_back();
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int y = q / nx + dy, x = q % nx + dx;
                    if (y < 0 || y >= ny || x < 0 || x >= nx) continue;
                    const int r = y * nx + x;
                    if (!labels[r] && (double)frame[r] > thr) {
                        labels[r] = n;
                        stack.push_back(r);
                    }
                }
        }
    }
    if (bad_rms)
        for (const Star& s : stars) {
            const size_t p = (size_t)s.y * nx + (size_t)s.x;
            rms[p] = (T)0;
            if (p + 1 < rms.size()) rms[p + 1] = (T)-1;
            if (p >= 1) rms[p - 1] = (T)__builtin_nan("");
        }
    std::vector<int32_t> boxes(4 * (size_t)(n + 1)), counts((size_t)n + 1), flags((size_t)n), eflags((size_t)n);
    std::vector<double> table((size_t)n * kMeasureCols), out((size_t)n * kErrorCols);
    emud_label_bboxes(labels.data(), ny, nx, n, boxes.data(), counts.data(), 3);
    int bad = n == expect ? 0 : 1;
    for (int pass = 0; pass < 2; ++pass) {
        const double gain = pass ? 2.5 : 0.0;
        measure<T>(frame.data(), nullptr, 0.01, nullptr, labels.data(), ny, nx, n, boxes.data(), table.data(),
                   flags.data(), 3);
        errors<T>(frame.data(), nullptr, 0.01, nullptr, 0.0, rms.data(), gain, labels.data(), ny, nx, n, boxes.data(),
                  table.data(), out.data(), eflags.data(), pass ? 64 : 1);
        for (int l = 0; l < n; ++l) {
            const double* o = out.data() + (size_t)l * kErrorCols;
            const double npix = table[(size_t)l * kMeasureCols];
            if (!(o[0] > 0.0) || !(o[1] >= 0.0) || !(o[2] >= 0.0) || o[3] * o[3] > o[1] * o[2] * (1.0 + 1e-9) ||
                !(o[4] >= 1.0 && o[4] <= npix) || o[5] != 2.0 * std::sqrt(o[4] / 3.14159265358979323846) ||
                ((eflags[l] & kErrFlagNoise) != 0) != bad_rms)
                ++bad;
            if (pass)
                std::printf("  %d: npix %.0f fluxerr %.6g errx2 %.3g erry2 %.3g nhalf %.0f fwhm %.4f eflags %d\n", l + 1,
                            npix, o[0], o[1], o[2], o[4], o[5], eflags[l]);
        }
    }
    std::printf("%s (%s): %d sources (expected %d)\n", what, sizeof(T) == 8 ? "float64" : "float32", n, expect);
    return bad;
}

template <typename T>
int all() {
    int bad = 0;
    bad += run<T>("stars", 72, 90, {{0, 0, 30, 2.0}, {20, 30, 50, 2.0}, {45, 55, 80, 6.0}, {71, 20, 20, 1.5}}, 0.7, true,
                  4);
    bad += run<T>("1 x 1 frame", 1, 1, {{0, 0, 3, 1.0}}, 0.7, false, 1);
    return bad;
}
}  // namespace

int main() {
    const int bad = all<float>() + all<double>();
    std::printf(bad ? "FAILED\n" : "OK\n");
    return bad ? 1 : 0;
}
