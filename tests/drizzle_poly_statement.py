"""The drizzle through polynomial maps of include/subpixal_hip.h stated a second time, independently of the kernel: a
forward SCATTER over input pixels in numpy float64 (the kernel is a gather with a candidate window; a scatter has no
window, so a candidate the kernel misses is a wrong pixel here).  Not a test module.

A map is a ``[6]`` affine or a ``resample.PolyMap``; either is re-expanded about the frame's centre in exact rational
arithmetic (``PolyMap.about``) and evaluated there as a plain sum of monomials (the kernel: extended precision and a
nested Horner scheme).  'square': the four corners (i -+ p/2, j -+ p/2) go through the map, the quadrilateral Q is
clipped against every output pixel its bounding box reaches by Sutherland-Hodgman in the PIXEL'S OWN coordinates
(``drizzle_statement.unit_square_overlap``), a = area / area(Q) with area(Q) by the shoelace formula.  'turbo': the
square of side p sqrt|det J| about M(i, j), J the analytic Jacobian.  'point': a = 1 on the pixel holding M(i, j).

BOUNDS, in the manner of drizzle_statement's, eps = 2^-53.  A computed output coordinate is within
(4 D + 3) eps S of the polynomial's value on the kernel's side (the header's evaluation order: 2 D roundings on the
longest Horner path, D ulps of S each for the rounding of u and of v, one for the rounded coefficient, two to spare),
S = sum |c(i, j) u^i v^j| at that point; this side's sum of monomials stays below the same count (a power by repeated
multiplication and the product with the coefficient: at most D + 1 roundings, the sum of up to 21 terms: 20 more, all
relative to partial sums <= S, so 4 D + 3 is replaced by D + 21 <= 26 here; the bound takes 4 D + 3 + 26).  So two
correct vertices differ by delta = (4 D + 29) eps Smax, Smax over the frame's corners, in place of the 4 eps Cmax of
the affine centre.  Moving every boundary point of Q by at most delta changes its overlap with a unit pixel by at most
4 delta (the boundary inside the pixel is at most the pixel's perimeter long) and area(Q) by at most perimeter(Q) delta.
After the vertices everything is local: numbers below 4 and fewer than 128 roundings per overlap on either side
(kernel: 4 edges of at most 20 with two divisions, 8 for the bounding box and the sum, 8 for area(Q); here as in
drizzle_statement).  With the per-drop 1 / area(Q) in place of the constant norm, two correct a differ by
    da = (4 delta + 2 * 128 * 4 eps + DROP_AREA + a perimeter(Q) delta + 16 eps) / area(Q)
and num, wht, sci follow as in drizzle_statement.  'turbo' adds the side's own error: det J from four derivative
sums, relative error (4 D + 29) eps Sj / |det| each, which moves the square's edges by s/2 of half that; it enters
delta.  The caps of ``drizzle_statement.check`` (faint pixels <= 1 %, grey ctx pairs < 1 %) are conditions on the
cases, verified on the statement alone in tests/test_drizzle_poly_cpu.py.
"""
import numpy as np

from drizzle_statement import DROP_AREA, EPS, KERNELS, check, ctx_bits, ctx_planes, effective_weight, unit_square_overlap

__all__ = ['statement', 'check', 'ctx_bits', 'ctx_planes', 'KERNELS', 'as_poly']


def as_poly(m):
    from subpixal_amd.resample import PolyMap
    return m if isinstance(m, PolyMap) else PolyMap.from_affine(np.asarray(m, np.float64))


def _abs_sum(m, x, y, du=0, dv=0):
    """sum |c u^i v^j| (or of the differentiated terms) per axis at the points (x, y), the larger of the two axes"""
    from subpixal_amd.resample import _TERMS
    u, v = np.abs(x - m.center[0]), np.abs(y - m.center[1])
    s = [np.zeros(np.shape(u)), np.zeros(np.shape(u))]
    for k, (i, j) in enumerate(_TERMS):
        if i + j > m.degree or i < du or j < dv:
            continue
        t = (i if du else 1) * (j if dv else 1) * u ** (i - du) * v ** (j - dv)
        s[0] = s[0] + abs(m.coef[0, k]) * t
        s[1] = s[1] + abs(m.coef[1, k]) * t
    return np.maximum(s[0], s[1])


def statement(frames, maps, out_shape, weights=None, masks=None, active=None, pixfrac=1.0, kernel='square',
              fill=0.0):
    K = len(frames)
    NY, NX = out_shape
    p = float(pixfrac)
    hp = 0.5 * p
    num, wht, sabs = np.zeros((NY, NX)), np.zeros((NY, NX)), np.zeros((NY, NX))
    tnum, twht, nterm = np.zeros((NY, NX)), np.zeros((NY, NX)), np.zeros((NY, NX))
    aw = np.zeros((K, NY, NX))
    wmax = 0.0
    for k in range(K):
        if active is not None and not active[k]:
            continue
        d = np.asarray(frames[k], np.float64)
        w = effective_weight(d, None if weights is None else weights[k], None if masks is None else masks[k])
        wmax = max(wmax, float(w.max()))
        ny, nx = d.shape
        m = as_poly(maps[k]).about((0.5 * (nx - 1), 0.5 * (ny - 1)))
        D = m.degree
        jj, ii = np.mgrid[0:ny, 0:nx].astype(np.float64)
        cnt = (4 * D + 29) * EPS
        if kernel == 'square':
            cu = [ii - hp, ii + hp, ii + hp, ii - hp]
            cv = [jj - hp, jj - hp, jj + hp, jj + hp]
            pts = [m(a, b) for a, b in zip(cu, cv)]
            delta = cnt * max(float(_abs_sum(m, a, b).max()) for a, b in zip(cu, cv))
        else:
            CX, CY = m(ii, jj)
            delta = cnt * float(_abs_sum(m, ii, jj).max())
            if kernel == 'turbo':
                J = m.jacobian(ii, jj)
                det = J[..., 0, 0] * J[..., 1, 1] - J[..., 0, 1] * J[..., 1, 0]
                hs = hp * np.sqrt(np.abs(det))
                sj = np.maximum(_abs_sum(m, ii, jj, du=1), _abs_sum(m, ii, jj, dv=1))
                # |d det| <= 4 Sj * (count eps Sj); d hs = hs / 2 * |d det| / |det|, plus the root and product
                delta += float((hs * (2.0 * cnt * sj * sj / np.abs(det) + 4 * EPS)).max())
                pts = [(CX - hs, CY - hs), (CX + hs, CY - hs), (CX + hs, CY + hs), (CX - hs, CY + hs)]
        idx, val = [], []
        for j in range(ny):
            for i in range(nx):
                wv = w[j, i]
                if wv == 0.0:
                    continue
                dv = d[j, i]
                if kernel == 'point':
                    X, Y = int(np.floor(CX[j, i] + 0.5)), int(np.floor(CY[j, i] + 0.5))
                    if 0 <= X < NX and 0 <= Y < NY:
                        idx.append((Y, X))
                        val.append((1.0, wv, dv, 0.0))
                    continue
                xs = [float(q[0][j, i]) for q in pts]
                ys = [float(q[1][j, i]) for q in pts]
                aq = 0.5 * abs((xs[2] - xs[0]) * (ys[3] - ys[1]) - (xs[3] - xs[1]) * (ys[2] - ys[0]))
                per = sum(np.hypot(xs[(q + 1) % 4] - xs[q], ys[(q + 1) % 4] - ys[q]) for q in range(4))
                X0, X1 = int(np.ceil(min(xs) - 0.5 - 1e-9)), int(np.floor(max(xs) + 0.5 + 1e-9))
                Y0, Y1 = int(np.ceil(min(ys) - 0.5 - 1e-9)), int(np.floor(max(ys) + 0.5 + 1e-9))
                for Y in range(max(Y0, 0), min(Y1, NY - 1) + 1):
                    for X in range(max(X0, 0), min(X1, NX - 1) + 1):
                        lx, ly = X - 0.5, Y - 0.5
                        a = unit_square_overlap([(x - lx, y - ly) for x, y in zip(xs, ys)]) / aq
                        da = (4.0 * delta + 1024.0 * EPS + DROP_AREA + a * per * delta + 16.0 * EPS) / aq
                        idx.append((Y, X))
                        val.append((a, wv, dv, da))
        if not idx:
            continue
        idx = np.array(idx)
        a, wv, dv, da = np.array(val).T
        at = (idx[:, 0], idx[:, 1])
        np.add.at(num, at, a * wv * dv)
        np.add.at(wht, at, a * wv)
        np.add.at(sabs, at, np.abs(a * wv * dv))
        np.add.at(tnum, at, da * wv * np.abs(dv))
        np.add.at(twht, at, da * wv)
        np.add.at(nterm, at, 1.0)
        np.add.at(aw[k], at, a * wv)
    bnum = tnum + (nterm + 4.0) * EPS * sabs
    bwht = twht + (nterm + 3.0) * EPS * wht
    filled = ~(wht > 0)
    with np.errstate(invalid='ignore', divide='ignore'):
        sci = np.where(filled, float(fill), num / wht)
    return dict(num=num, wht=wht, sci=sci, filled=filled, aw=aw, wmax=wmax, bnum=bnum, bwht=bwht, K=K)
