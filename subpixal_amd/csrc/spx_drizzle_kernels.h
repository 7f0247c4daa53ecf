// spx_drizzle_kernels.h -- the forward resampler ("drizzle", Fruchter & Hook 2002) for affine maps: what the
// reference's resample.py gets from drizzlepac.  One kernel, drizzle_kernel<T>, and the host function that packs the
// per-frame rows it reads (host::drizzle_pack_row).  Needs spx_rt_hip.h (or the CPU harness) first.
//
// DEFINITION (include/subpixal_hip.h carries it in full; tests/drizzle_statement.py states it in numpy as a scatter)
//   Pixel (i, j) is centred on integer coordinates.  Frame k maps input to output pixels by
//   (X, Y) = (a0 x + a1 y + a2, a3 x + a4 y + a5).  The drop of input pixel (i, j) is the square of side pixfrac p
//   centred on it.  An input pixel has effective weight 0 when it is masked, its value or its weight is not finite,
//   or its weight is <= 0.
//     kernel 0 'square': a = area(M(drop) n P_XY) / (|det A| p^2)
//     kernel 1 'turbo' : M(drop) replaced by the axis-aligned square of side p sqrt|det A| centred on M(i, j)
//     kernel 2 'point' : a = 1 for the pixel (floor(X + 1/2), floor(Y + 1/2)) that holds M(i, j), else 0
//   num = sum a w d, wht = sum a w over active frames k ascending, then j ascending, then i ascending, in float64
//   with contraction off; sci = num / wht where wht > 0, else fill; ctx bit k is set iff frame k added a w > 0.
//
// GATHER.  One thread owns one output pixel and its two accumulators across all frames: no atomics, and the order
// of the sum is the definition's, so the result is the same bit pattern on every run and for every grid size.  For
// output pixel (X, Y) and frame k the candidates are the input pixels within (rx, ry) of c = A^-1((X, Y) - t),
// with rx = |A^-1_00| hx + |A^-1_01| hy, hx = p/2 (|a0| + |a1|) + 1/2 (ry, hy likewise): every pixel whose drop can
// touch P_XY.  A workgroup owns a 32 x 8 output tile and skips, as one, a frame whose pixels all lie outside the
// tile's candidate range.  The frames are read with plain global loads: neighbouring lanes read neighbouring
// pixels, and the 9 .. 25-fold reuse between neighbouring output pixels is left to the caches.
//
// OVERLAP for 'square': the signed area under each of the four edges of M(drop), clipped to the unit pixel, in
// PIXEL-LOCAL coordinates ((X - 1/2, Y - 1/2) subtracted first); the absolute value of the sum, which makes a
// mirrored map come out right.  All four edges of every drop of a frame share two slopes: they are in the row, and
// there is no division per pixel.
#pragma once

#include <math.h>
#include <stdint.h>

namespace spx {

constexpr int kDrzTileW = 32, kDrzTileH = 8;     // output pixels per workgroup of 256
constexpr int kDrzMaxFrames = 128;
constexpr int kDrzMaxWindow = 8;                 // candidates per axis the host accepts
// an overlap below this area (output pixels^2) is rounding noise of the four edge terms, which cancel only to a few
// ulp when Q misses the pixel: it is dropped, so that a pixel no drop reaches stays at `fill`
constexpr double kDrzDropArea = 1e-12;
constexpr int kDrzSquare = 0, kDrzTurbo = 1, kDrzPoint = 2;

// One frame as the kernel reads it: 28 eight-byte fields (SPX_DRIZZLE_ROW_BYTES = 224).
struct DrizzleRow {
    const void* data;          // [ny][nx] in the frame dtype
    const void* weight;        // same shape and dtype, or null: weight 1
    const uint8_t* mask;       // same shape, nonzero = bad, or null
    int32_t ny, nx;
    int32_t active, reserved;
    double a[6];               // the forward map
    double inv[4];             // A^-1, row-major
    double rx, ry;             // half-sides of the candidate window
    double bx, by;             // half-sides of the mapped drop's bounding box
    double inv_norm;           // 1 / (|det A| p^2)
    double e[4];               // 'square': the drop's two edge vectors e1 = p (a0, a3), e2 = p (a1, a4)
    double m[2], im[2];        // their slopes dy/dx and dx/dy (0 where the other is infinite or the edge is flat)
};
static_assert(sizeof(DrizzleRow) == 224, "DrizzleRow is part of the C ABI");

namespace host {
// Fills `r` for one frame.  Returns 0, or 1: a map entry is not finite, 2: the map is singular, 3: the candidate
// window exceeds kDrzMaxWindow.
inline int drizzle_pack_row(const void* data, const void* weight, const uint8_t* mask, int ny, int nx, int active,
                            const double* a, double p, int kernel, DrizzleRow* r) {
#pragma clang fp contract(off)
    for (int q = 0; q < 6; ++q)
        if (!(a[q] - a[q] == 0.0)) return 1;
    const double det = a[0] * a[4] - a[1] * a[3];
    const double big = fmax(fmax(fabs(a[0]), fabs(a[1])), fmax(fabs(a[3]), fabs(a[4])));
    if (!(fabs(det) > 1e-12 * big * big) || !(1.0 / det - 1.0 / det == 0.0)) return 2;
    r->data = data;
    r->weight = weight;
    r->mask = mask;
    r->ny = ny;
    r->nx = nx;
    r->active = active ? 1 : 0;
    r->reserved = 0;
    for (int q = 0; q < 6; ++q) r->a[q] = a[q];
    r->inv[0] = a[4] / det;
    r->inv[1] = -a[1] / det;
    r->inv[2] = -a[3] / det;
    r->inv[3] = a[0] / det;
    const double adet = fabs(det);
    if (kernel == kDrzSquare) {
        r->bx = 0.5 * p * (fabs(a[0]) + fabs(a[1]));
        r->by = 0.5 * p * (fabs(a[3]) + fabs(a[4]));
    } else if (kernel == kDrzTurbo) {
        r->bx = r->by = 0.5 * p * sqrt(adet);
    } else {
        r->bx = r->by = 0.0;
    }
    const double hx = r->bx + 0.5, hy = r->by + 0.5;
    // (the 1e-9 keeps a pixel whose drop only touches P_XY inside the window whatever the rounding of c: it adds 0)
    r->rx = fabs(r->inv[0]) * hx + fabs(r->inv[1]) * hy + 1e-9;
    r->ry = fabs(r->inv[2]) * hx + fabs(r->inv[3]) * hy + 1e-9;
    if (!(2.0 * r->rx + 1.0 <= (double)kDrzMaxWindow) || !(2.0 * r->ry + 1.0 <= (double)kDrzMaxWindow)) return 3;
    r->inv_norm = 1.0 / (adet * (p * p));
    r->e[0] = p * a[0];
    r->e[1] = p * a[3];
    r->e[2] = p * a[1];
    r->e[3] = p * a[4];
    for (int q = 0; q < 2; ++q) {
        const double dx = r->e[2 * q], dy = r->e[2 * q + 1];
        r->m[q] = dx != 0.0 ? dy / dx : 0.0;
        r->im[q] = dy != 0.0 ? dx / dy : 0.0;
    }
    return 0;
}
}  // namespace host

// The signed area between the edge (x1, y1) -> (x2, y2) and the x axis, clipped to the unit square [0, 1]^2;
// m = dy/dx and im = dx/dy of the edge.  Positive when the edge runs towards +x.
SPX_DEVICE double drz_edge_area(double x1, double y1, double x2, double y2, double m, double im) {
#pragma clang fp contract(off)
    if (x1 == x2) return 0.0;                    // a vertical edge has nothing under it
    double sign = 1.0;
    if (x1 > x2) {
        const double tx = x1, ty = y1;
        x1 = x2; y1 = y2; x2 = tx; y2 = ty;
        sign = -1.0;
    }
    double xlo = x1 > 0.0 ? x1 : 0.0, xhi = x2 < 1.0 ? x2 : 1.0;
    if (!(xlo < xhi)) return 0.0;
    double ylo = x1 > 0.0 ? y1 : y1 + m * (0.0 - x1);
    double yhi = x2 < 1.0 ? y2 : y1 + m * (1.0 - x1);
    if (ylo <= 0.0 && yhi <= 0.0) return 0.0;
    if (ylo >= 1.0 && yhi >= 1.0) return sign * (xhi - xlo);
    double area = 0.0;
    if (ylo < 0.0) {                             // enters through y = 0: nothing before the crossing
        xlo = xlo + (0.0 - ylo) * im;
        ylo = 0.0;
    } else if (ylo > 1.0) {                      // above the pixel up to the crossing of y = 1: a full-height strip
        const double xc = xlo + (1.0 - ylo) * im;
        area = xc - xlo;
        xlo = xc;
        ylo = 1.0;
    }
    if (yhi < 0.0) {
        xhi = xhi + (0.0 - yhi) * im;
        yhi = 0.0;
    } else if (yhi > 1.0) {
        const double xc = xhi + (1.0 - yhi) * im;
        area += xhi - xc;
        xhi = xc;
        yhi = 1.0;
    }
    area += 0.5 * (ylo + yhi) * (xhi - xlo);
    return sign * area;
}

// a of the definition for the drop centred on (cx, cy) in the local coordinates of the output pixel [0, 1]^2
SPX_DEVICE double drz_overlap(const DrizzleRow& r, int kernel, double cx, double cy) {
#pragma clang fp contract(off)
    if (cx + r.bx <= 0.0 || cx - r.bx >= 1.0 || cy + r.by <= 0.0 || cy - r.by >= 1.0) return 0.0;
    if (kernel == kDrzTurbo) {
        const double x0 = cx - r.bx > 0.0 ? cx - r.bx : 0.0, x1 = cx + r.bx < 1.0 ? cx + r.bx : 1.0;
        const double y0 = cy - r.by > 0.0 ? cy - r.by : 0.0, y1 = cy + r.by < 1.0 ? cy + r.by : 1.0;
        const double ar = (x1 - x0) * (y1 - y0);
        return ar > kDrzDropArea ? ar * r.inv_norm : 0.0;
    }
    const double h1x = 0.5 * r.e[0], h1y = 0.5 * r.e[1], h2x = 0.5 * r.e[2], h2y = 0.5 * r.e[3];
    const double v0x = (cx - h1x) - h2x, v0y = (cy - h1y) - h2y;
    const double v1x = (cx + h1x) - h2x, v1y = (cy + h1y) - h2y;
    const double v2x = (cx + h1x) + h2x, v2y = (cy + h1y) + h2y;
    const double v3x = (cx - h1x) + h2x, v3y = (cy - h1y) + h2y;
    double s = drz_edge_area(v0x, v0y, v1x, v1y, r.m[0], r.im[0]);
    s += drz_edge_area(v1x, v1y, v2x, v2y, r.m[1], r.im[1]);
    s += drz_edge_area(v2x, v2y, v3x, v3y, r.m[0], r.im[0]);
    s += drz_edge_area(v3x, v3y, v0x, v0y, r.m[1], r.im[1]);
    const double ar = fabs(s);
    return ar > kDrzDropArea ? ar * r.inv_norm : 0.0;
}

// The frame against a 32 x 8 output tile (centre (tcx, tcy), half-sides (thx, thy), in output pixels): the inverse
// image of the tile's bounding box, grown by the window (and by one pixel against the rounding of the centre), is
// compared with the frame as a whole.  True: no pixel of the frame reaches any pixel of the tile.
SPX_DEVICE bool drz_frame_misses_tile(const DrizzleRow& r, double tcx, double tcy, double thx, double thy) {
#pragma clang fp contract(off)
    const double ux = tcx - r.a[2], uy = tcy - r.a[5];
    const double ccx = r.inv[0] * ux + r.inv[1] * uy, ccy = r.inv[2] * ux + r.inv[3] * uy;
    const double ex = fabs(r.inv[0]) * thx + fabs(r.inv[1]) * thy + r.rx + 1.0;
    const double ey = fabs(r.inv[2]) * thx + fabs(r.inv[3]) * thy + r.ry + 1.0;
    return ccx + ex < 0.0 || ccx - ex > (double)(r.nx - 1) || ccy + ey < 0.0 || ccy - ey > (double)(r.ny - 1);
}

// Adds frame r's terms for output pixel (X, Y) to num and den in the definition's order (j ascending, then i
// ascending); true iff one of them had a w > 0.  drizzle_kernel carries num and den across the frames,
// drizzle_median_kernel (spx_crreject_kernels.h) starts every frame from 0.
template <typename T>
SPX_DEVICE bool drz_frame_sums(const DrizzleRow& r, int kernel, int X, int Y, double& num, double& den) {
#pragma clang fp contract(off)
    const double ux = (double)X - r.a[2], uy = (double)Y - r.a[5];
    const double px = r.inv[0] * ux + r.inv[1] * uy, py = r.inv[2] * ux + r.inv[3] * uy;
    int i0 = (int)ceil(fmax(px - r.rx, -1.0)), i1 = (int)floor(fmin(px + r.rx, (double)r.nx));
    int j0 = (int)ceil(fmax(py - r.ry, -1.0)), j1 = (int)floor(fmin(py + r.ry, (double)r.ny));
    if (i0 < 0) i0 = 0;
    if (j0 < 0) j0 = 0;
    if (i1 > r.nx - 1) i1 = r.nx - 1;
    if (j1 > r.ny - 1) j1 = r.ny - 1;
    const T* __restrict__ D = static_cast<const T*>(r.data);
    const T* __restrict__ W = static_cast<const T*>(r.weight);
    const double lx = (double)X - 0.5, ly = (double)Y - 0.5;
    bool hit = false;
    for (int j = j0; j <= j1; ++j) {
        for (int i = i0; i <= i1; ++i) {
            // the drop's centre in the output, then in the pixel's own coordinates
            const double CX = (r.a[0] * (double)i + r.a[1] * (double)j) + r.a[2];
            const double CY = (r.a[3] * (double)i + r.a[4] * (double)j) + r.a[5];
            const double a = kernel == kDrzPoint
                                 ? (floor(CX + 0.5) == (double)X && floor(CY + 0.5) == (double)Y ? 1.0 : 0.0)
                                 : drz_overlap(r, kernel, CX - lx, CY - ly);
            if (!(a > 0.0)) continue;
            const int64_t q = (int64_t)j * r.nx + i;
            const T d = D[q];
            if (!(d - d == T(0)) || (r.mask && r.mask[q])) continue;
            double w = 1.0;
            if (W) {
                const T wv = W[q];
                if (!(wv - wv == T(0)) || !(wv > T(0))) continue;
                w = (double)wv;
            }
            const double aw = a * w;
            num += aw * (double)d;
            den += aw;
            if (aw > 0.0) hit = true;
        }
    }
    return hit;
}

template <typename T>
SPX_TKERNEL(256)
void drizzle_kernel(const DrizzleRow* __restrict__ rows, int nframes, int kernel, double fill, int out_ny, int out_nx,
                    T* __restrict__ sci, float* __restrict__ wht, int32_t* __restrict__ ctx) {
#pragma clang fp contract(off)
    const int tid = rt::thread_id();
    const int64_t tiles_x = (out_nx + kDrzTileW - 1) / kDrzTileW, tiles_y = (out_ny + kDrzTileH - 1) / kDrzTileH;
    const int64_t plane = (int64_t)out_ny * out_nx;
    for (int64_t tile = rt::block_id(); tile < tiles_x * tiles_y; tile += rt::grid_size()) {
        const int X0 = (int)(tile % tiles_x) * kDrzTileW, Y0 = (int)(tile / tiles_x) * kDrzTileH;
        const int X = X0 + (tid & (kDrzTileW - 1)), Y = Y0 + tid / kDrzTileW;
        const bool inside = X < out_nx && Y < out_ny;
        const int64_t o = (int64_t)Y * out_nx + X;
        // the tile's centre and half-sides, in output pixels
        const double tcx = (double)X0 + 0.5 * (kDrzTileW - 1), tcy = (double)Y0 + 0.5 * (kDrzTileH - 1);
        const double thx = 0.5 * (kDrzTileW - 1), thy = 0.5 * (kDrzTileH - 1);
        double num = 0.0, den = 0.0;
        uint32_t word = 0;
        for (int k = 0; k < nframes; ++k) {
            if (k && !(k & 31)) {
                if (inside) ctx[(int64_t)((k >> 5) - 1) * plane + o] = (int32_t)word;
                word = 0;
            }
            const DrizzleRow& r = rows[k];
            if (!r.active) continue;
            if (drz_frame_misses_tile(r, tcx, tcy, thx, thy)) continue;
            if (!inside) continue;
            if (drz_frame_sums<T>(r, kernel, X, Y, num, den)) word |= 1u << (k & 31);
        }
        if (inside) {
            ctx[(int64_t)((nframes - 1) >> 5) * plane + o] = (int32_t)word;
            sci[o] = den > 0.0 ? (T)(num / den) : (T)fill;
            wht[o] = (float)den;
        }
    }
}

}  // namespace spx
