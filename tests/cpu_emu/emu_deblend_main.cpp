// TEST INFRASTRUCTURE ONLY: a stand-alone program over emu_deblend.cpp for a sanitizer pass on the CPU (the
// harness allocates LDS and the workspace slots with exactly the sizes of the real launches, so an address
// sanitizer reports any access beyond them).  Build and run, from the repository root:
//   clang++ -std=c++20 -O1 -g -pthread -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -Isubpixal_amd/csrc -Itests/cpu_emu -o /tmp/emu_deblend_main tests/cpu_emu/emu_deblend_main.cpp
//   /tmp/emu_deblend_main            (or -fsanitize=thread instead)
// It draws four scenes -- one parent per storage class: one wave, LDS, workspace, over the box limit --, labels
// them with a plain flood fill, runs the deblending in float32 and float64 and prints the segment counts.
#include "emu_deblend.cpp"

#include <cstdio>

namespace {
struct Star { double y, x, amp, sigma; };

template <typename T>
int run(const char* what, int ny, int nx, const std::vector<Star>& stars, double ring, double thr, bool filter,
        int expect) {
    std::vector<T> frame((size_t)ny * nx, T(0));
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            double v = 0.0;
            for (const Star& s : stars)
                v += s.amp * std::exp(-((y - s.y) * (y - s.y) + (x - s.x) * (x - s.x)) / (2.0 * s.sigma * s.sigma));
            if (ring > 0.0 && y >= 10 && y < ny - 10 && x >= 10 && x < nx - 10 &&
                (y == 10 || y == ny - 11 || x == 10 || x == nx - 11))
                v += ring + ((x == 60 || x == 200) && y == 10 ? 40.0 : 0.0);
            frame[(size_t)y * nx + x] = (T)(std::floor(v * 64.0) / 64.0);
        }
    // labels 1..n in raster order of the first pixel, 8-connected, on the unfiltered frame
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
    std::vector<int32_t> boxes(4 * (size_t)(n + 1));
    for (int l = 0; l <= n; ++l) {
        boxes[4 * l] = boxes[4 * l + 1] = 0x7fffffff;
        boxes[4 * l + 2] = boxes[4 * l + 3] = -1;
    }
    for (int p = 0; p < ny * nx; ++p) {
        const int l = labels[p];
        if (!l) continue;
        boxes[4 * l] = std::min(boxes[4 * l], p % nx);
        boxes[4 * l + 1] = std::min(boxes[4 * l + 1], p / nx);
        boxes[4 * l + 2] = std::max(boxes[4 * l + 2], p % nx);
        boxes[4 * l + 3] = std::max(boxes[4 * l + 3], p / nx);
    }
    const T box[9] = {T(0.125), T(0.125), T(0.125), T(0.125), T(0.125), T(0.125), T(0.125), T(0.125), T(0.125)};
    const int max_out = 64;
    std::vector<int32_t> out((size_t)ny * nx), parent(max_out), dflags(max_out);
    int32_t nout = -5;
    for (int mode = 0; mode < 2; ++mode)
        for (int conn = 4; conn <= 8; conn += 4)
            deblend<T>(frame.data(), nullptr, filter ? box : nullptr, 3, 3, ny, nx, labels.data(), n, boxes.data(), conn,
                       5, 31, 0.005, mode, out.data(), parent.data(), dflags.data(), max_out, &nout, 3, kDebLdsPixels);
    std::printf("%s (%s): %d parents -> %d segments (expected %d)\n", what, sizeof(T) == 8 ? "float64" : "float32", n,
                nout, expect);
    return nout == expect ? 0 : 1;
}

template <typename T>
int all() {
    int bad = 0;
    bad += run<T>("one wave", 24, 30, {{11, 10, 100, 1.0}, {11, 16, 90, 1.0}}, 0.0, 0.7, true, 2);
    bad += run<T>("LDS", 40, 57, {{19, 22, 100, 2.5}, {20, 34, 80, 2.5}}, 0.0, 0.7, true, 2);
    bad += run<T>("workspace", 160, 161, {{60, 55, 100, 12}, {95, 100, 80, 12}, {65, 120, 30, 8}}, 0.0, 0.7, false, 3);
    bad += run<T>("over the limit", 281, 283, {{140, 130, 100, 2.5}, {141, 142, 100, 2.5}}, 5.0, 0.7, false, 3);
    return bad;
}
}  // namespace

int main() {
    const int bad = all<float>() + all<double>();
    std::printf(bad ? "FAILED\n" : "OK\n");
    return bad ? 1 : 0;
}
