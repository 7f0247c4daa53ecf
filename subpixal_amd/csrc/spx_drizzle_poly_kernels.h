// spx_drizzle_poly_kernels.h -- the forward resampler of spx_drizzle_kernels.h for frames whose map to the output grid
// is a bivariate polynomial of total degree 1 .. 5 (instrument distortion): drizzle_poly_kernel<T> and the host
// function that packs the per-frame rows it reads (host::drizzle_poly_pack_row).  Needs spx_drizzle_kernels.h first.
//
// DEFINITION (include/subpixal_hip.h carries it in full; tests/drizzle_poly_statement.py states it in numpy as a
// scatter).  Everything of the affine drizzle stands -- pixel convention, effective weight, accumulation order,
// float64 with contraction off, sci = num / wht, fill, ctx, the 1e-12 px^2 drop threshold, no scale^2 -- but the map:
//   u = x - xc, v = y - yc;  X = sum_{d=0..degree} sum_{i=d..0} coef[0][k] u^i v^(d-i),  k = d (d + 1) / 2 + (d - i),
//   Y likewise with coef[1][k]                                    (the 21 slots and the order of spx_blot_poly4_f32)
//     'square': Q = the quadrilateral with straight edges through M(i -+ p/2, j -+ p/2) (cyclic order);
//               a = |area(Q n P_XY)| / |area(Q)|
//     'turbo' : the axis-aligned square of side s = p sqrt|det J(i, j)| centred on M(i, j); a = overlap / (s s)
//     'point' : a = 1 on the pixel (floor(X + 1/2), floor(Y + 1/2)) that holds M(i, j)
//
// EVALUATION ORDER.  The host re-expands the map about the FRAME'S centre (xf, yf) = ((nx - 1) / 2, (ny - 1) / 2), in
// extended precision, and rounds every coefficient once; the kernel never sees the caller's centre, so a map given
// about a far centre loses nothing.  A point is (u, v) = ((i - xf) +- p/2, (j - yf) +- p/2): the difference is exact,
// the half drop one rounding.  The value is a nested Horner scheme, by powers of v outside and of u inside:
//     acc = c(0, D);  for j = D-1 .. 0 { r = c(D-j, j); for i = D-j-1 .. 0: r = r u + c(i, j);  acc = acc v + r }
// with c(i, j) the coefficient of u^i v^j: D (D + 3) / 2 multiply-add pairs (20 at degree 5), and no coefficient
// passes through more than 2 D roundings.  With the rounding of (u, v) themselves (each costs at most D ulps of the
// sum of the terms) and of the coefficients, a computed coordinate is within (4 D + 3) eps sum |c(i, j) u^i v^j| of
// the polynomial's value.
//
// GATHER.  As drizzle_kernel<T>: one thread per output pixel, 32 x 8 tiles of 256 threads, two float64 accumulators
// carried across the frames, no atomics, a whole-tile skip of a frame that cannot reach the tile.  Per output pixel T
// and frame the kernel estimates c ~ M^-1(T) by `steps` chord iterations c <- c - A^-1 (M(c) - T) from
// c0 = A^-1 (T - M(centre)), A = J(centre), and visits the input pixels within (rx, ry) of c.  For every candidate the
// overlap is computed FROM THE FORWARD MAP OF THAT CANDIDATE'S OWN CORNERS: the estimate only selects candidates.
//
// WHY NO DROP WITH A NON-ZERO OVERLAP FALLS OUTSIDE THE WINDOW.  Let the domain be the frame grown by a margin m, and
// over it (sums of |coefficient| times the monomials' largest values, so true bounds, not samples)
//     dN >= |A^-1 J - 1| entrywise,  R >= |A^-1 (M - its linearisation at the centre)|  (both from the coefficients
//     of A^-1 M, so a rotation costs nothing),  sag >= p^2 / 8 max(|M_uu|, |M_vv|),  B = |A^-1| entrywise,
//     rho = the largest row sum of dN  (refused unless rho < 1/2).
// rho < 1 makes M one-to-one on the domain (M(a) - M(b) = Jm (a - b) with |1 - A^-1 Jm| <= rho), so the image of a
// drop is a curved quadrilateral whose edges lie within sag of the chords of Q.  If pixel q's drop overlaps P_T there
// is therefore a point p of the drop (|p - q| <= s = p/2 per axis) with |M(p) - T| <= h = 1/2 + sag per axis.  ('turbo':
// p = q, s = 0 and h = 1/2 + p/2 sqrt(max |det J|); 'point': p = q, s = 0, h = 1/2.)  For that p,
//     c0 - p = A^-1 (T - M(p)) + A^-1 (M(p) - lin(p)),            so |c0 - p| <= B h + R             =: e0,
//     c' - p = (1 - A^-1 Jm) (c - p) - A^-1 (M(p) - T),           so |c' - p| <= rho |c - p|_max + B h,
// Jm the mean Jacobian between p and c; every iterate stays within max(e0, |B h| / (1 - rho)) of p, inside the
// domain as the host checks m >= s + that.  After n steps, per axis,
//     |c - q| <= (B h)_axis + rho / (1 - rho) |B h|_max + rho^n |e0|_max + s  (+ 1e-9 for the roundings)  =: (rx, ry).
// The tile skip uses the n = 0 form: |c0 - q| <= e0 + s =: (ex, ey), and c0 is affine in T.
//
// OVERLAP for 'square': the signed area under each of the four edges of Q clipped to the unit pixel, in pixel-local
// coordinates, as drz_edge_area, but the slopes are the edge's own: an edge divides only where it really crosses
// x = 0 or 1 (dy / dx, once) or y = 0 or 1 (dx / dy, once).  At pixfrac 1 neighbouring drops share corners, and
// (i - xf) + 1/2 = (i + 1 - xf) - 1/2 exactly, so a candidate takes its left corners from its left neighbour:
// bit-identical to evaluating them again.
#pragma once

#include <math.h>
#include <stdint.h>

namespace spx {

constexpr int kDrzPolyTerms = 21;
constexpr int kDrzPolyMaxDegree = 5;
constexpr int kDrzPolyMaxSteps = 6;
constexpr int kDrzPolyLattice = 33;              // the determinant is checked on 33 x 33 positions (see pack_row)

// One frame as the kernel reads it: 61 eight-byte fields (SPX_DRIZZLE_POLY_ROW_BYTES = 488).  The first 40 bytes are
// those of DrizzleRow.
struct DrizzlePolyRow {
    const void* data;          // [ny][nx] in the frame dtype
    const void* weight;        // same shape and dtype, or null: weight 1
    const uint8_t* mask;       // same shape, nonzero = bad, or null
    int32_t ny, nx;
    int32_t active, reserved;
    double coef[2][kDrzPolyTerms];   // the map about (xc, yc); slots above the degree are 0
    double xc, yc;             // the frame's centre ((nx - 1) / 2, (ny - 1) / 2)
    double inv[4];             // A^-1, A = J(xc, yc), row-major
    double rx, ry;             // half-sides of the candidate window
    double ex, ey;             // reach of the linear estimate c0 (the tile skip)
    double bx, by;             // bounds, over the frame, of the half-sides of a drop's bounding box in the output:
                               // they size the window, and 'turbo' rejects a candidate by them before its Jacobian
    double hp;                 // pixfrac / 2
    int32_t degree, steps;     // 1 .. 5; chord iterations of the inverse estimate
};
static_assert(sizeof(DrizzlePolyRow) == 488, "DrizzlePolyRow is part of the C ABI");

constexpr int drzp_slot(int i, int j) { return (i + j) * (i + j + 1) / 2 + j; }      // of u^i v^j

namespace host {
// sum over the terms of degree dmin .. D of |c| * |d^du_u d^dv_v (u^i v^j)| at (U, V): a bound over |u| <= U, |v| <= V
inline double drzp_abs_bound(const double* c, int D, int du, int dv, double U, double V, int dmin) {
    double s = 0.0;
    for (int d = dmin; d <= D; ++d)
        for (int j = 0; j <= d; ++j) {
            const int i = d - j;
            if (i < du || j < dv) continue;
            double f = 1.0;
            for (int q = 0; q < du; ++q) f *= (double)(i - q);
            for (int q = 0; q < dv; ++q) f *= (double)(j - q);
            s += fabs(c[drzp_slot(i, j)]) * f * pow(U, (double)(i - du)) * pow(V, (double)(j - dv));
        }
    return s;
}
// d^du_u d^dv_v of the polynomial at (u, v), du + dv <= 1
inline double drzp_value(const double* c, int D, int du, int dv, double u, double v) {
    double s = 0.0;
    for (int d = D; d >= 0; --d)
        for (int j = 0; j <= d; ++j) {
            const int i = d - j;
            if (i < du || j < dv) continue;
            const double f = (du ? (double)i : 1.0) * (dv ? (double)j : 1.0);
            s += c[drzp_slot(i, j)] * f * pow(u, (double)(i - du)) * pow(v, (double)(j - dv));
        }
    return s;
}

// Fills `r` for one frame.  Returns 0, or 1: a used coefficient or the centre is not finite, 2: the Jacobian
// determinant is zero, not finite or of both signs on the lattice, 3: the candidate window exceeds kDrzMaxWindow (or
// the Jacobian varies so much that no window can be given: rho >= 1/2), 4: degree outside 1 .. 5.
// The lattice: kDrzPolyLattice x kDrzPolyLattice positions, evenly spaced from -1/2 to nx - 1/2 and from -1/2 to
// ny - 1/2 (the frame's border, its corners and, as node (16, 16), its centre).
inline int drizzle_poly_pack_row(const void* data, const void* weight, const uint8_t* mask, int ny, int nx, int active,
                                 const double* coef, int degree, const double* center, double p, int kernel,
                                 DrizzlePolyRow* r) {
#pragma clang fp contract(off)
    if (degree < 1 || degree > kDrzPolyMaxDegree) return 4;
    const int D = degree, nterms = (D + 1) * (D + 2) / 2;
    for (int a = 0; a < 2; ++a) {
        if (!(center[a] - center[a] == 0.0)) return 1;
        for (int k = 0; k < nterms; ++k)
            if (!(coef[a * kDrzPolyTerms + k] - coef[a * kDrzPolyTerms + k] == 0.0)) return 1;
    }
    // the map about the frame's centre: u = u' + sx, so u^i v^j = sum C(i, a) C(j, b) sx^(i-a) sy^(j-b) u'^a v'^b
    const double xf = 0.5 * (double)(nx - 1), yf = 0.5 * (double)(ny - 1);
    const long double sx = (long double)xf - (long double)center[0], sy = (long double)yf - (long double)center[1];
    static const double binom[6][6] = {{1, 0, 0, 0, 0, 0}, {1, 1, 0, 0, 0, 0},  {1, 2, 1, 0, 0, 0},
                                       {1, 3, 3, 1, 0, 0}, {1, 4, 6, 4, 1, 0}, {1, 5, 10, 10, 5, 1}};
    long double px[6] = {1, 0, 0, 0, 0, 0}, py[6] = {1, 0, 0, 0, 0, 0};
    for (int q = 1; q <= D; ++q) {
        px[q] = px[q - 1] * sx;
        py[q] = py[q - 1] * sy;
    }
    double cc[2][kDrzPolyTerms];
    for (int a = 0; a < 2; ++a) {
        long double acc[kDrzPolyTerms];
        for (int k = 0; k < kDrzPolyTerms; ++k) acc[k] = 0.0L;
        for (int d = 0; d <= D; ++d)
            for (int j = 0; j <= d; ++j) {
                const int i = d - j;
                const long double c = (long double)coef[a * kDrzPolyTerms + drzp_slot(i, j)];
                for (int ia = 0; ia <= i; ++ia)
                    for (int jb = 0; jb <= j; ++jb)
                        acc[drzp_slot(ia, jb)] += c * (long double)binom[i][ia] * (long double)binom[j][jb] *
                                                  px[i - ia] * py[j - jb];
            }
        for (int k = 0; k < kDrzPolyTerms; ++k) {
            cc[a][k] = (double)acc[k];
            if (!(cc[a][k] - cc[a][k] == 0.0)) return 1;
        }
    }
    // the determinant on the lattice
    const double U0 = 0.5 * (double)nx, V0 = 0.5 * (double)ny;
    int sign = 0;
    for (int b = 0; b < kDrzPolyLattice; ++b)
        for (int a = 0; a < kDrzPolyLattice; ++a) {
            const double u = U0 * ((double)(2 * a) / (double)(kDrzPolyLattice - 1) - 1.0);
            const double v = V0 * ((double)(2 * b) / (double)(kDrzPolyLattice - 1) - 1.0);
            const double j00 = drzp_value(cc[0], D, 1, 0, u, v), j01 = drzp_value(cc[0], D, 0, 1, u, v);
            const double j10 = drzp_value(cc[1], D, 1, 0, u, v), j11 = drzp_value(cc[1], D, 0, 1, u, v);
            const double det = j00 * j11 - j01 * j10;
            const double big = fmax(fmax(fabs(j00), fabs(j01)), fmax(fabs(j10), fabs(j11)));
            if (!(fabs(det) > 1e-12 * big * big) || !(1.0 / det - 1.0 / det == 0.0)) return 2;
            const int s = det > 0.0 ? 1 : -1;
            if (sign && s != sign) return 2;
            sign = s;
        }
    const double a00 = cc[0][1], a01 = cc[0][2], a10 = cc[1][1], a11 = cc[1][2];
    const double det = a00 * a11 - a01 * a10;
    const double inv[4] = {a11 / det, -a01 / det, -a10 / det, a00 / det};
    const double B[4] = {fabs(inv[0]), fabs(inv[1]), fabs(inv[2]), fabs(inv[3])};
    const double s_in = kernel == kDrzSquare ? 0.5 * p : 0.0;
    double nc[2][kDrzPolyTerms];                     // the coefficients of A^-1 M
    for (int a = 0; a < 2; ++a)
        for (int k = 0; k < kDrzPolyTerms; ++k) nc[a][k] = inv[2 * a] * cc[0][k] + inv[2 * a + 1] * cc[1][k];
    double m = 2.0, rho = 0.0, e0 = 0.0, Bh[2] = {0.0, 0.0}, BhR[2] = {0.0, 0.0}, bx = 0.0, by = 0.0;
    bool settled = false;
    for (int it = 0; it < 16 && !settled; ++it) {
        const double U = U0 + m, V = V0 + m;
        double dJ[4], dN[4], R[2], h[2];
        for (int a = 0; a < 2; ++a) {
            dJ[2 * a] = drzp_abs_bound(cc[a], D, 1, 0, U, V, 2);
            dJ[2 * a + 1] = drzp_abs_bound(cc[a], D, 0, 1, U, V, 2);
            dN[2 * a] = drzp_abs_bound(nc[a], D, 1, 0, U, V, 2);
            dN[2 * a + 1] = drzp_abs_bound(nc[a], D, 0, 1, U, V, 2);
            R[a] = drzp_abs_bound(nc[a], D, 0, 0, U, V, 2);
        }
        rho = fmax(dN[0] + dN[1], dN[2] + dN[3]);
        if (!(rho < 0.5)) return 3;
        const double g00 = fabs(a00) + dJ[0], g01 = fabs(a01) + dJ[1], g10 = fabs(a10) + dJ[2], g11 = fabs(a11) + dJ[3];
        if (kernel == kDrzSquare) {
            for (int a = 0; a < 2; ++a)
                h[a] = 0.5 + 0.125 * p * p * fmax(drzp_abs_bound(cc[a], D, 2, 0, U, V, 2),
                                                  drzp_abs_bound(cc[a], D, 0, 2, U, V, 2));
            bx = 0.5 * p * (g00 + g01) + (h[0] - 0.5);
            by = 0.5 * p * (g10 + g11) + (h[1] - 0.5);
        } else if (kernel == kDrzTurbo) {
            bx = by = 0.5 * p * sqrt(g00 * g11 + g01 * g10);
            h[0] = h[1] = 0.5 + bx;
        } else {
            bx = by = 0.0;
            h[0] = h[1] = 0.5;
        }
        for (int a = 0; a < 2; ++a) {
            Bh[a] = B[2 * a] * h[0] + B[2 * a + 1] * h[1];
            BhR[a] = Bh[a] + R[a];
        }
        e0 = fmax(BhR[0], BhR[1]);
        const double need = s_in + fmax(e0, fmax(Bh[0], Bh[1]) / (1.0 - rho)) + 0.01;
        if (!(need - need == 0.0)) return 3;
        if (need <= m) settled = true;
        else m = need + 0.5;
    }
    if (!settled) return 3;
    int steps = 0;
    double tail = 0.0;
    // (a degree-1 map has rho = 0 and R = 0: c0 is the inverse, and no step is taken)
    if (rho > 0.0)
        for (tail = rho * e0, steps = 1; tail > 0.01 && steps < kDrzPolyMaxSteps; ++steps) tail *= rho;
    const double spread = rho / (1.0 - rho) * fmax(Bh[0], Bh[1]);
    const double rx = Bh[0] + spread + tail + s_in + 1e-9, ry = Bh[1] + spread + tail + s_in + 1e-9;
    if (!(2.0 * rx + 1.0 <= (double)kDrzMaxWindow) || !(2.0 * ry + 1.0 <= (double)kDrzMaxWindow)) return 3;
    r->data = data;
    r->weight = weight;
    r->mask = mask;
    r->ny = ny;
    r->nx = nx;
    r->active = active ? 1 : 0;
    r->reserved = 0;
    for (int a = 0; a < 2; ++a)
        for (int k = 0; k < kDrzPolyTerms; ++k) r->coef[a][k] = cc[a][k];
    r->xc = xf;
    r->yc = yf;
    for (int q = 0; q < 4; ++q) r->inv[q] = inv[q];
    r->rx = rx;
    r->ry = ry;
    r->ex = BhR[0] + s_in + 1e-9;
    r->ey = BhR[1] + s_in + 1e-9;
    r->bx = bx;
    r->by = by;
    r->hp = 0.5 * p;
    r->degree = D;
    r->steps = steps;
    return 0;
}
}  // namespace host

// the polynomial with coefficients c (21 slots) at (u, v): the header's nested Horner scheme, unrolled for degree D
template <int D>
SPX_DEVICE double drzp_eval(const double* __restrict__ c, double u, double v) {
#pragma clang fp contract(off)
    double acc = c[drzp_slot(0, D)];
#pragma unroll
    for (int j = D - 1; j >= 0; --j) {
        double r = c[drzp_slot(D - j, j)];
#pragma unroll
        for (int i = D - j - 1; i >= 0; --i) r = r * u + c[drzp_slot(i, j)];
        acc = acc * v + r;
    }
    return acc;
}
// its derivatives by u and by v, the same scheme over the differentiated coefficients
template <int D>
SPX_DEVICE double drzp_eval_du(const double* __restrict__ c, double u, double v) {
#pragma clang fp contract(off)
    double acc = 0.0;
#pragma unroll
    for (int j = D - 1; j >= 0; --j) {
        double r = (double)(D - j) * c[drzp_slot(D - j, j)];
#pragma unroll
        for (int i = D - j - 1; i >= 1; --i) r = r * u + (double)i * c[drzp_slot(i, j)];
        acc = acc * v + r;
    }
    return acc;
}
template <int D>
SPX_DEVICE double drzp_eval_dv(const double* __restrict__ c, double u, double v) {
#pragma clang fp contract(off)
    double acc = (double)D * c[drzp_slot(0, D)];
#pragma unroll
    for (int j = D - 1; j >= 1; --j) {
        double r = c[drzp_slot(D - j, j)];
#pragma unroll
        for (int i = D - j - 1; i >= 0; --i) r = r * u + c[drzp_slot(i, j)];
        acc = acc * v + (double)j * r;
    }
    return acc;
}

// drz_edge_area for an edge with slopes of its own: the signed area between the edge (x1, y1) -> (x2, y2) and the x
// axis, clipped to [0, 1]^2.  It divides once if the edge crosses x = 0 or x = 1 and once if it crosses y = 0 or 1.
SPX_DEVICE double drzp_edge_area(double x1, double y1, double x2, double y2) {
#pragma clang fp contract(off)
    if (x1 == x2) return 0.0;
    double sign = 1.0;
    if (x1 > x2) {
        const double tx = x1, ty = y1;
        x1 = x2; y1 = y2; x2 = tx; y2 = ty;
        sign = -1.0;
    }
    if (!(x2 > 0.0) || !(x1 < 1.0)) return 0.0;
    const double dx = x2 - x1, dy = y2 - y1;
    double xlo = x1, ylo = y1, xhi = x2, yhi = y2;
    if (x1 < 0.0 || x2 > 1.0) {
        const double m = dy / dx;
        if (x1 < 0.0) {
            ylo = y1 + m * (0.0 - x1);
            xlo = 0.0;
        }
        if (x2 > 1.0) {
            yhi = y1 + m * (1.0 - x1);
            xhi = 1.0;
        }
    }
    if (!(xlo < xhi)) return 0.0;
    if (ylo <= 0.0 && yhi <= 0.0) return 0.0;
    if (ylo >= 1.0 && yhi >= 1.0) return sign * (xhi - xlo);
    double area = 0.0;
    if (ylo < 0.0 || ylo > 1.0 || yhi < 0.0 || yhi > 1.0) {
        const double im = dx / dy;                   // the ends differ in y here, so dy != 0
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
    }
    area += 0.5 * (ylo + yhi) * (xhi - xlo);
    return sign * area;
}

// True: no pixel of the frame reaches any pixel of the tile (centre (tcx, tcy), half-sides (thx, thy), output pixels).
SPX_DEVICE bool drzp_frame_misses_tile(const DrizzlePolyRow& r, double tcx, double tcy, double thx, double thy) {
#pragma clang fp contract(off)
    const double dx = tcx - r.coef[0][0], dy = tcy - r.coef[1][0];
    const double ccx = (r.inv[0] * dx + r.inv[1] * dy) + r.xc, ccy = (r.inv[2] * dx + r.inv[3] * dy) + r.yc;
    const double ex = fabs(r.inv[0]) * thx + fabs(r.inv[1]) * thy + r.ex + 1.0;
    const double ey = fabs(r.inv[2]) * thx + fabs(r.inv[3]) * thy + r.ey + 1.0;
    return ccx + ex < 0.0 || ccx - ex > (double)(r.nx - 1) || ccy + ey < 0.0 || ccy - ey > (double)(r.ny - 1);
}

// Adds frame r's terms for output pixel (X, Y) to num and den in the definition's order; true iff one had a w > 0.
template <typename T, int D>
SPX_DEVICE bool drzp_frame_sums(const DrizzlePolyRow& r, int kernel, int X, int Y, double& num, double& den) {
#pragma clang fp contract(off)
    const double* __restrict__ cx = r.coef[0];
    const double* __restrict__ cy = r.coef[1];
    const double tx = (double)X, ty = (double)Y;
    double eu, ev;
    {
        const double dx = tx - cx[0], dy = ty - cy[0];
        eu = r.inv[0] * dx + r.inv[1] * dy;
        ev = r.inv[2] * dx + r.inv[3] * dy;
    }
    for (int s = 0; s < r.steps; ++s) {
        const double fx = drzp_eval<D>(cx, eu, ev) - tx, fy = drzp_eval<D>(cy, eu, ev) - ty;
        eu = eu - (r.inv[0] * fx + r.inv[1] * fy);
        ev = ev - (r.inv[2] * fx + r.inv[3] * fy);
    }
    const double px = eu + r.xc, py = ev + r.yc;
    // an estimate that ran away belongs to a pixel the frame cannot reach (see the header: a reached pixel's stays
    // within e0 / (1 - rho) of the frame)
    if (!(fabs(px) < 1e9) || !(fabs(py) < 1e9)) return false;
    int i0 = (int)ceil(fmax(px - r.rx, -1.0)), i1 = (int)floor(fmin(px + r.rx, (double)r.nx));
    int j0 = (int)ceil(fmax(py - r.ry, -1.0)), j1 = (int)floor(fmin(py + r.ry, (double)r.ny));
    if (i0 < 0) i0 = 0;
    if (j0 < 0) j0 = 0;
    if (i1 > r.nx - 1) i1 = r.nx - 1;
    if (j1 > r.ny - 1) j1 = r.ny - 1;
    const T* __restrict__ Dt = static_cast<const T*>(r.data);
    const T* __restrict__ W = static_cast<const T*>(r.weight);
    const double lx = tx - 0.5, ly = ty - 0.5;
    const double hp = r.hp;
    const bool share = hp == 0.5;
    bool hit = false;
    for (int j = j0; j <= j1; ++j) {
        const double v = (double)j - r.yc;
        double sx1 = 0.0, sy1 = 0.0, sx2 = 0.0, sy2 = 0.0;           // the right corners of the previous candidate
        for (int i = i0; i <= i1; ++i) {
            const double u = (double)i - r.xc;
            double a = 0.0;
            if (kernel == kDrzSquare) {
                const double u0 = u - hp, u1 = u + hp, v0 = v - hp, v1 = v + hp;
                double x0, y0, x3, y3;
                if (share && i > i0) {
                    x0 = sx1; y0 = sy1; x3 = sx2; y3 = sy2;
                } else {
                    x0 = drzp_eval<D>(cx, u0, v0) - lx; y0 = drzp_eval<D>(cy, u0, v0) - ly;
                    x3 = drzp_eval<D>(cx, u0, v1) - lx; y3 = drzp_eval<D>(cy, u0, v1) - ly;
                }
                const double x1 = drzp_eval<D>(cx, u1, v0) - lx, y1 = drzp_eval<D>(cy, u1, v0) - ly;
                const double x2 = drzp_eval<D>(cx, u1, v1) - lx, y2 = drzp_eval<D>(cy, u1, v1) - ly;
                sx1 = x1; sy1 = y1; sx2 = x2; sy2 = y2;
                const double xmin = fmin(fmin(x0, x1), fmin(x2, x3)), xmax = fmax(fmax(x0, x1), fmax(x2, x3));
                const double ymin = fmin(fmin(y0, y1), fmin(y2, y3)), ymax = fmax(fmax(y0, y1), fmax(y2, y3));
                if (xmax <= 0.0 || xmin >= 1.0 || ymax <= 0.0 || ymin >= 1.0) continue;
                double s = drzp_edge_area(x0, y0, x1, y1);
                s += drzp_edge_area(x1, y1, x2, y2);
                s += drzp_edge_area(x2, y2, x3, y3);
                s += drzp_edge_area(x3, y3, x0, y0);
                const double ar = fabs(s);
                if (ar > kDrzDropArea) {
                    const double aq = 0.5 * fabs((x2 - x0) * (y3 - y1) - (x3 - x1) * (y2 - y0));
                    a = ar / aq;
                }
            } else {
                const double CX = drzp_eval<D>(cx, u, v), CY = drzp_eval<D>(cy, u, v);
                if (kernel == kDrzPoint) {
                    a = floor(CX + 0.5) == tx && floor(CY + 0.5) == ty ? 1.0 : 0.0;
                } else {
                    const double mx = CX - lx, my = CY - ly;
                    // (bx, by) bound the square's half-side over the whole frame: a centre further than that from
                    // the pixel needs no Jacobian
                    const double gx = r.bx + 1e-9, gy = r.by + 1e-9;
                    if (mx + gx <= 0.0 || mx - gx >= 1.0 || my + gy <= 0.0 || my - gy >= 1.0) continue;
                    const double det = drzp_eval_du<D>(cx, u, v) * drzp_eval_dv<D>(cy, u, v) -
                                       drzp_eval_dv<D>(cx, u, v) * drzp_eval_du<D>(cy, u, v);
                    const double hs = hp * sqrt(fabs(det));
                    if (mx + hs <= 0.0 || mx - hs >= 1.0 || my + hs <= 0.0 || my - hs >= 1.0) continue;
                    const double xa = mx - hs > 0.0 ? mx - hs : 0.0, xb = mx + hs < 1.0 ? mx + hs : 1.0;
                    const double ya = my - hs > 0.0 ? my - hs : 0.0, yb = my + hs < 1.0 ? my + hs : 1.0;
                    const double ar = (xb - xa) * (yb - ya);
                    const double side = 2.0 * hs;
                    if (ar > kDrzDropArea) a = ar / (side * side);
                }
            }
            if (!(a > 0.0)) continue;
            const int64_t q = (int64_t)j * r.nx + i;
            const T d = Dt[q];
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
void drizzle_poly_kernel(const DrizzlePolyRow* __restrict__ rows, int nframes, int kernel, double fill, int out_ny,
                         int out_nx, T* __restrict__ sci, float* __restrict__ wht, int32_t* __restrict__ ctx) {
#pragma clang fp contract(off)
    const int tid = rt::thread_id();
    const int64_t tiles_x = (out_nx + kDrzTileW - 1) / kDrzTileW, tiles_y = (out_ny + kDrzTileH - 1) / kDrzTileH;
    const int64_t plane = (int64_t)out_ny * out_nx;
    for (int64_t tile = rt::block_id(); tile < tiles_x * tiles_y; tile += rt::grid_size()) {
        const int X0 = (int)(tile % tiles_x) * kDrzTileW, Y0 = (int)(tile / tiles_x) * kDrzTileH;
        const int X = X0 + (tid & (kDrzTileW - 1)), Y = Y0 + tid / kDrzTileW;
        const bool inside = X < out_nx && Y < out_ny;
        const int64_t o = (int64_t)Y * out_nx + X;
        const double tcx = (double)X0 + 0.5 * (kDrzTileW - 1), tcy = (double)Y0 + 0.5 * (kDrzTileH - 1);
        const double thx = 0.5 * (kDrzTileW - 1), thy = 0.5 * (kDrzTileH - 1);
        double num = 0.0, den = 0.0;
        uint32_t word = 0;
        for (int k = 0; k < nframes; ++k) {
            if (k && !(k & 31)) {
                if (inside) ctx[(int64_t)((k >> 5) - 1) * plane + o] = (int32_t)word;
                word = 0;
            }
            const DrizzlePolyRow& r = rows[k];
            if (!r.active) continue;
            if (drzp_frame_misses_tile(r, tcx, tcy, thx, thy)) continue;
            if (!inside) continue;
            bool hit = false;
            switch (r.degree) {                      // the degree is the frame's: uniform, and the loops unroll
                case 1: hit = drzp_frame_sums<T, 1>(r, kernel, X, Y, num, den); break;
                case 2: hit = drzp_frame_sums<T, 2>(r, kernel, X, Y, num, den); break;
                case 3: hit = drzp_frame_sums<T, 3>(r, kernel, X, Y, num, den); break;
                case 4: hit = drzp_frame_sums<T, 4>(r, kernel, X, Y, num, den); break;
                default: hit = drzp_frame_sums<T, 5>(r, kernel, X, Y, num, den); break;
            }
            if (hit) word |= 1u << (k & 31);
        }
        if (inside) {
            ctx[(int64_t)((nframes - 1) >> 5) * plane + o] = (int32_t)word;
            sci[o] = den > 0.0 ? (T)(num / den) : (T)fill;
            wht[o] = (float)den;
        }
    }
}

}  // namespace spx
