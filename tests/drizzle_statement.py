"""The drizzle of include/subpixal_hip.h stated a second time, independently of the kernel: a forward SCATTER over
input pixels in numpy float64 (the kernel is a gather over output pixels).  Not a test module.

For every input pixel with effective weight > 0 the drop's image Q (a parallelogram for 'square', an axis-aligned
square for 'turbo') is clipped against each output pixel its bounding box reaches by Sutherland-Hodgman, in the
PIXEL'S OWN coordinates (the pixel is [0, 1]^2: absolute coordinates cost 6e-11 at x ~ 4000, local ones 2e-14), and
the area is the shoelace formula's.  a = area / (|det A| p^2).  np.add.at accumulates num = sum a w d and
wht = sum a w.  'point' puts a = 1 on the pixel (floor(X + 1/2), floor(Y + 1/2)).

BOUNDS.  eps = 2^-53.  Both sides compute the drop's centre C = (a0 i + a1 j) + a2 in 4 roundings of numbers no larger
than Cmax (the largest coordinate in play), so each is within 4 eps Cmax of the true centre; moving a drop by delta
changes its overlap with a unit pixel by at most 4 delta (the boundary of Q inside the pixel is at most the pixel's
perimeter long).  After the centre everything is local: numbers below 4, and fewer than 64 roundings per overlap
on either side (kernel: 16 for the corners, 4 x 11 per edge, 4 for the sum; here: 8 intersections of 6, shoelace of
3 per vertex for at most 8 vertices).  So two correct overlaps differ by at most
    dA = eps (2 * 4 * 4 Cmax + 2 * 64 * 4) = eps (32 Cmax + 512)            (area, output pixels^2)
and the kernel may drop an overlap below 1e-12 as rounding noise (DROP_AREA).  a = A / norm adds 2 roundings, a w one,
a w d one, and a sum of n terms n - 1 more, each relative to the running sum <= S = sum |a w d|:
    |num - num'| <= (dA + DROP_AREA) sum_touch(w |d|) / norm + (n + 4) eps S
    |wht - wht'| <= (dA + DROP_AREA) sum_touch(w) / norm + (n + 3) eps sum(a w)
where sum_touch runs over the drops whose bounding box reaches the pixel.  sci = num / wht:
    |sci - sci'| <= (bnum + |sci| bwht) / (wht - bwht) + eps |sci| + u |sci|,   u = the output dtype's half-ulp,
used where wht > 2 bwht; elsewhere sci is not compared (check() asserts that this is under 1 % of the pixels).
"""
import numpy as np

EPS = 2.0 ** -53
DROP_AREA = 1e-12
KERNELS = {'square': 0, 'turbo': 1, 'point': 2}


def _clip(poly, axis, bound, keep_less):
    """Sutherland-Hodgman against one edge of the unit square"""
    out = []
    n = len(poly)
    for q in range(n):
        p0, p1 = poly[q], poly[(q + 1) % n]
        in0 = p0[axis] <= bound if keep_less else p0[axis] >= bound
        in1 = p1[axis] <= bound if keep_less else p1[axis] >= bound
        if in0 != in1:
            t = (bound - p0[axis]) / (p1[axis] - p0[axis])
            x = [p0[0] + t * (p1[0] - p0[0]), p0[1] + t * (p1[1] - p0[1])]
            x[axis] = bound
            if in0:
                out.append(p0)
            out.append(tuple(x))
        elif in0:
            out.append(p0)
    return out


def unit_square_overlap(poly):
    """area of the convex polygon `poly` (a list of (x, y)) inside [0, 1]^2"""
    for axis, bound, less in ((0, 0.0, False), (0, 1.0, True), (1, 0.0, False), (1, 1.0, True)):
        poly = _clip(poly, axis, bound, less)
        if len(poly) < 3:
            return 0.0
    s = 0.0
    for q in range(len(poly)):
        x0, y0 = poly[q]
        x1, y1 = poly[(q + 1) % len(poly)]
        s += x0 * y1 - x1 * y0
    return abs(s) / 2.0


def effective_weight(d, w, m):
    d = np.asarray(d, np.float64)
    ww = np.ones_like(d) if w is None else np.asarray(w, np.float64).copy()
    bad = ~np.isfinite(d) | ~np.isfinite(ww) | ~(ww > 0)
    if m is not None:
        bad |= np.asarray(m) != 0
    ww[bad] = 0.0
    return ww


def statement(frames, maps, out_shape, weights=None, masks=None, active=None, pixfrac=1.0, kernel='square',
              fill=0.0):
    K = len(frames)
    NY, NX = out_shape
    p = float(pixfrac)
    num = np.zeros((NY, NX))
    wht = np.zeros((NY, NX))
    sabs = np.zeros((NY, NX))
    tnum = np.zeros((NY, NX))
    twht = np.zeros((NY, NX))
    nterm = np.zeros((NY, NX))
    aw = np.zeros((K, NY, NX))
    cmax = float(max(NY, NX))
    wmax = 0.0
    for k in range(K):
        if active is not None and not active[k]:
            continue
        d = np.asarray(frames[k], np.float64)
        w = effective_weight(d, None if weights is None else weights[k], None if masks is None else masks[k])
        wmax = max(wmax, float(w.max()))
        a0, a1, a2, a3, a4, a5 = [float(v) for v in maps[k]]
        det = a0 * a4 - a1 * a3
        norm = abs(det) * p * p
        ny, nx = d.shape
        cmax = max(cmax, ny, nx, abs(a0) * nx + abs(a1) * ny + abs(a2), abs(a3) * nx + abs(a4) * ny + abs(a5))
        if kernel == 'turbo':
            h = 0.5 * p * np.sqrt(abs(det))
            offs = ((-h, -h), (h, -h), (h, h), (-h, h))
        else:
            e1 = (0.5 * p * a0, 0.5 * p * a3)
            e2 = (0.5 * p * a1, 0.5 * p * a4)
            offs = ((-e1[0] - e2[0], -e1[1] - e2[1]), (e1[0] - e2[0], e1[1] - e2[1]),
                    (e1[0] + e2[0], e1[1] + e2[1]), (-e1[0] + e2[0], -e1[1] + e2[1]))
        idx, val = [], []
        for j in range(ny):
            for i in range(nx):
                wv = w[j, i]
                if wv == 0.0:
                    continue
                dv = d[j, i]
                cx = (a0 * i + a1 * j) + a2
                cy = (a3 * i + a4 * j) + a5
                if kernel == 'point':
                    X, Y = int(np.floor(cx + 0.5)), int(np.floor(cy + 0.5))
                    if 0 <= X < NX and 0 <= Y < NY:
                        idx.append((Y, X))
                        val.append((1.0, wv, dv, 0.0))
                    continue
                xs = [cx + o[0] for o in offs]
                ys = [cy + o[1] for o in offs]
                X0, X1 = int(np.ceil(min(xs) - 0.5 - 1e-9)), int(np.floor(max(xs) + 0.5 + 1e-9))
                Y0, Y1 = int(np.ceil(min(ys) - 0.5 - 1e-9)), int(np.floor(max(ys) + 0.5 + 1e-9))
                for Y in range(max(Y0, 0), min(Y1, NY - 1) + 1):
                    for X in range(max(X0, 0), min(X1, NX - 1) + 1):
                        lx, ly = X - 0.5, Y - 0.5
                        poly = [(x - lx, y - ly) for x, y in zip(xs, ys)]
                        idx.append((Y, X))
                        val.append((unit_square_overlap(poly) / norm, wv, dv, 1.0 / norm))
        if not idx:
            continue
        idx = np.array(idx)
        a, wv, dv, inorm = np.array(val).T
        at = (idx[:, 0], idx[:, 1])
        np.add.at(num, at, a * wv * dv)
        np.add.at(wht, at, a * wv)
        np.add.at(sabs, at, np.abs(a * wv * dv))
        np.add.at(tnum, at, inorm * wv * np.abs(dv))
        np.add.at(twht, at, inorm * wv)
        np.add.at(nterm, at, 1.0)
        np.add.at(aw[k], at, a * wv)
    dA = EPS * (32.0 * cmax + 512.0) + DROP_AREA
    bnum = dA * tnum + (nterm + 4.0) * EPS * sabs
    bwht = dA * twht + (nterm + 3.0) * EPS * wht
    filled = ~(wht > 0)
    with np.errstate(invalid='ignore', divide='ignore'):
        sci = np.where(filled, float(fill), num / wht)
    return dict(num=num, wht=wht, sci=sci, filled=filled, aw=aw, wmax=wmax, bnum=bnum, bwht=bwht, K=K)


def ctx_planes(bits):
    """bool [K][NY][NX] -> int32 [ceil(K / 32)][NY][NX]"""
    K = bits.shape[0]
    out = np.zeros(((K + 31) // 32,) + bits.shape[1:], np.uint32)
    for k in range(K):
        out[k // 32] |= bits[k].astype(np.uint32) << np.uint32(k % 32)
    return out.view(np.int32)


def ctx_bits(ctx, K):
    u = np.ascontiguousarray(ctx).view(np.uint32)
    return np.stack([(u[k // 32] >> np.uint32(k % 32)) & np.uint32(1) for k in range(K)]).astype(bool)


def check(sci, wht, ctx, st, what=''):
    """an implementation's outputs against statement()'s: wht and sci within the bounds (num is no output of the
    library: it is covered through sci and wht), the fill pattern exactly, ctx outside the grey zone.

    ctx: the bit must be set where the statement's a w > 1e-9 max w and clear where the statement's overlap is exactly
    0 (which holds wherever the drop's bounding box, grown by 1e-9, misses the pixel, and further where only the box
    touches it).  Pairs in between are skipped and must be under 1 % of the (pixel, frame) pairs."""
    K = st['K']
    assert sci.shape == st['sci'].shape and wht.shape == sci.shape and wht.dtype == np.float32, what
    assert ctx.dtype == np.int32 and ctx.shape == ((K + 31) // 32,) + sci.shape, what
    got_filled = ~(wht > 0)
    assert np.array_equal(got_filled, st['filled']), '%s: fill pattern differs at %d pixels' % (
        what, int((got_filled != st['filled']).sum()))
    u = 2.0 ** -24 if sci.dtype == np.float32 else EPS
    ew = np.abs(wht.astype(np.float64) - st['wht'])
    bw = st['bwht'] + 2.0 ** -24 * st['wht']
    assert np.all(ew <= bw), '%s: wht off by %g (bound %g)' % (what, ew.max(), bw[np.argmax(ew - bw)])
    ok = st['wht'] > 2.0 * st['bwht']
    assert np.array_equal(sci[st['filled']].astype(np.float64), st['sci'][st['filled']]), what
    skipped = (~ok & ~st['filled']).sum()
    assert skipped <= 0.01 * sci.size, '%s: %d pixels too faint to compare' % (what, skipped)
    with np.errstate(invalid='ignore', divide='ignore'):
        bs = (st['bnum'] + np.abs(st['sci']) * st['bwht']) / (st['wht'] - st['bwht']) + (EPS + u) * np.abs(st['sci'])
    es = np.abs(sci.astype(np.float64) - st['sci'])
    assert np.all(es[ok] <= bs[ok]), '%s: sci off by %g (bound %g)' % (what, es[ok].max(),
                                                                        bs[ok][np.argmax(es[ok] - bs[ok])])
    bits = ctx_bits(ctx, K)
    must = st['aw'] > 1e-9 * st['wmax']
    clear = st['aw'] == 0.0
    assert np.all(bits[must]), '%s: ctx bits missing' % what
    assert not np.any(bits[clear]), '%s: ctx bits set where nothing lands' % what
    grey = (~must & ~clear).sum()
    assert grey < 0.01 * must.size, '%s: grey zone %d of %d' % (what, grey, must.size)
    # bits beyond frame K - 1 are zero
    if K % 32:
        assert not np.any(np.ascontiguousarray(ctx).view(np.uint32)[-1] >> np.uint32(K % 32)), what
    return dict(wht_err=float(ew.max()), sci_err=float(es[ok].max()) if ok.any() else 0.0, grey=int(grey))
