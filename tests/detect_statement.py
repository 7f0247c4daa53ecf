"""The CPU statement of source finding that tests/test_detect_cpu.py and tests/test_gpu_detect.py compare
against: numpy/scipy in float64, independent of the code under test (scipy.ndimage.correlate for the filter,
`>` for the mask, scipy.ndimage.label for the components, np.bincount for areas and moments), and the checks
with their derived bounds.  Not a test module itself."""
import numpy as np
from scipy import ndimage

COLS = ('npix', 'flux', 'x', 'y', 'x2', 'y2', 'xy', 'a', 'b', 'theta', 'peak', 'xpeak', 'ypeak')
U = 2.0 ** -52
THETA_CUT = 1e-3            # theta is undefined for a == b: not compared where (a - b) / a is below this
THETA_SKIP_CAP = 0.05       # ... which may happen to at most 5 % of a scene's sources

STRUCT = {8: np.ones((3, 3), int), 4: np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])}


def detection(frame, thr, mask=None, filt=None):
    """(detected, tie): the mask in float64, and the pixels whose filtered value lies within
    64 eps(dtype) sum|k v| of the threshold, which float32 arithmetic could legitimately flip"""
    v = np.asarray(frame, np.float64)
    ok = np.isfinite(v)
    if mask is not None:
        ok &= ~np.asarray(mask, bool)
    vp = np.where(ok, v, 0.0)
    if filt is None:
        f, mag = vp, np.abs(vp)
    else:
        k = np.asarray(filt, np.float64)
        f = ndimage.correlate(vp, k, mode='constant', cval=0.0)
        mag = ndimage.correlate(np.abs(vp), np.abs(k), mode='constant', cval=0.0)
    t = np.asarray(thr, np.float64)
    eps = float(np.finfo(np.asarray(frame).dtype).eps)
    tie = ok & (np.abs(f - t) <= 64 * eps * np.maximum(mag, np.abs(t)))
    return ok & (f > t), tie, ok


def statement(frame, thr, bkg=0.0, mask=None, filt=None, min_area=1, conn=8):
    det, tie, ok = detection(frame, thr, mask, filt)
    # a test-construction error, not a failure of the code under test: rebuild the scene
    assert not tie.any(), "scene has %d pixels within rounding of the threshold" % tie.sum()
    lab, n = ndimage.label(det, structure=STRUCT[conn])
    area = np.bincount(lab.ravel(), minlength=n + 1)
    keep = area >= min_area
    keep[0] = False
    newid = np.where(keep, np.cumsum(keep), 0).astype(np.int32)
    lab = newid[lab]
    n = int(keep.sum())
    ny, nx = lab.shape
    sel = lab > 0
    l = lab[sel] - 1
    ys, xs = np.nonzero(sel)
    w = (np.asarray(frame, np.float64) - np.asarray(bkg, np.float64) * np.ones(lab.shape))[sel]
    xmin = np.full(n, nx); xmax = np.full(n, -1); ymin = np.full(n, ny); ymax = np.full(n, -1)
    np.minimum.at(xmin, l, xs); np.maximum.at(xmax, l, xs); np.minimum.at(ymin, l, ys); np.maximum.at(ymax, l, ys)
    dx, dy = (xs - xmin[l]).astype(np.float64), (ys - ymin[l]).astype(np.float64)
    terms = [w, w * dx, w * dy, w * (dx * dx), w * (dy * dy), w * (dx * dy)]
    S = [np.bincount(l, weights=t, minlength=n) for t in terms]
    A = [np.bincount(l, weights=np.abs(t), minlength=n) for t in terms]
    npix = np.bincount(l, minlength=n)
    # peak: first maximum in raster order
    lin = ys.astype(np.int64) * nx + xs
    order = np.lexsort((lin, -w, l))
    first = order[np.r_[True, l[order][1:] != l[order][:-1]]] if len(l) else order
    peak, xpeak, ypeak = w[first], xs[first].astype(np.float64), ys[first].astype(np.float64)
    # flags
    badsum = np.pad(np.cumsum(np.cumsum(~ok, 0), 1), ((1, 0), (1, 0)))
    inbox = (badsum[ymax + 1, xmax + 1] - badsum[ymin, xmax + 1] - badsum[ymax + 1, xmin] + badsum[ymin, xmin]) > 0
    flux = S[0]
    flags = ((xmin == 0) | (ymin == 0) | (xmax == nx - 1) | (ymax == ny - 1)).astype(np.int32)
    flags |= 2 * (flux <= 0) | 4 * inbox
    with np.errstate(all='ignore'):
        pos = flux > 0
        F = np.where(pos, flux, np.nan)
        mx, my = S[1] / F, S[2] / F
        x, y = xmin + mx, ymin + my
        x2, y2, xy = S[3] / F - mx * mx, S[4] / F - my * my, S[5] / F - mx * my
        hs, hd = 0.5 * (x2 + y2), 0.5 * (x2 - y2)
        rad = np.sqrt(hd * hd + xy * xy)
        a, b = np.sqrt(np.maximum(hs + rad, 0.0)), np.sqrt(np.maximum(hs - rad, 0.0))
        theta = 0.5 * np.degrees(np.arctan2(2.0 * xy, x2 - y2))
        # ---- bounds.  Each sum: both sides add npix terms in float64 in SOME order, each within
        # (npix - 1) 2^-53 sum|term| of the exact sum, the products' own roundings another 2^-53 sum|term|:
        # |delta| <= npix 2^-52 sum|term|.
        bS = [npix * U * t for t in A]
        # every later operation (+ - * / sqrt) rounds once on each side: 2 * 2^-53 = U relative to its result,
        # allowed as 4 U on the magnitudes involved (atan2 on the device is not correctly rounded: 8 U there).
        # ratio r = S/F: |dr| <= dS/F + |S| dF/F^2 to first order; scenes keep dF <= 1e-3 F (asserted), the
        # second-order remainder is covered by the factor 1.01.
        assert np.all(bS[0][pos] <= 1e-3 * flux[pos]), "scene has a source whose flux cancels"
        def ratio(i):
            return 1.01 * (bS[i] / F + np.abs(S[i]) * bS[0] / F ** 2) + 4 * U * np.abs(S[i] / F)
        dmx, dmy = ratio(1), ratio(2)
        bx, by = dmx + 4 * U * np.abs(x), dmy + 4 * U * np.abs(y)
        bx2 = ratio(3) + 2.02 * np.abs(mx) * dmx + 8 * U * (np.abs(S[3] / F) + mx * mx)
        by2 = ratio(4) + 2.02 * np.abs(my) * dmy + 8 * U * (np.abs(S[4] / F) + my * my)
        bxy = ratio(5) + 1.01 * (np.abs(mx) * dmy + np.abs(my) * dmx) + 8 * U * (np.abs(S[5] / F) + np.abs(mx * my))
        # hs, hd: halves of sums; rad = hypot(hd, xy): |d rad| <= |d hd| + |d xy| (unit gradient components)
        bhs = 0.5 * (bx2 + by2) + 4 * U * (np.abs(x2) + np.abs(y2))
        brad = bhs + bxy + 8 * U * rad
        b2 = bhs + brad + 4 * U * (np.abs(hs) + rad)             # bound of a^2 and of b^2
        # |sqrt u - sqrt u'| <= |u - u'| / sqrt(u) and <= sqrt|u - u'|
        tiny = np.finfo(np.float64).tiny                          # one pixel: a = b = 0 exactly, bound 0
        ba = b2 / np.maximum(np.maximum(a, np.sqrt(b2)), tiny) + 4 * U * a
        bb = b2 / np.maximum(np.maximum(b, np.sqrt(b2)), tiny) + 4 * U * b
        # theta = atan2(N, D) / 2, N = 2 xy, D = x2 - y2, N^2 + D^2 = 4 rad^2: |d theta| <= (|D| dN + |N| dD) /
        # (2 (N^2 + D^2)) <= (2 dxy + dD) / (4 rad) radians
        bth = np.degrees((2 * bxy + bx2 + by2 + 8 * U * (np.abs(x2) + np.abs(y2))) / (4 * rad)) + 8 * U * 90.0
    tab = dict(npix=npix.astype(np.float64), flux=flux, x=x, y=y, x2=x2, y2=y2, xy=xy, a=a, b=b, theta=theta,
               peak=peak, xpeak=xpeak, ypeak=ypeak)
    bound = dict(flux=bS[0], x=bx, y=by, x2=bx2, y2=by2, xy=bxy, a=ba, b=bb, theta=bth)
    bbox = np.stack([xmin, ymin, xmax, ymax], axis=1).astype(np.int32)
    return dict(labels=lab.astype(np.int32), n=n, table=tab, bound=bound, flags=flags, bbox=bbox)


def check(got_labels, got_table, got_flags, got_bbox, st, what='', verbose=True):
    """got_table [n, 13] float64 in COLS order, got_bbox [n, 4] (xmin, ymin, xmax, ymax).
    Labels, npix, bbox, peak position, flags, peak: exact.  Sums and what derives from them: the bounds above."""
    assert got_labels.shape == st['labels'].shape
    nd = int((got_labels != st['labels']).sum())
    assert nd == 0, "%s: label image differs from scipy's at %d pixels (labels %d vs %d)" % (
        what, nd, got_labels.max(initial=0), st['n'])
    n = st['n']
    assert got_table.shape == (n, len(COLS)) and got_flags.shape == (n,)
    if n == 0:
        return dict(n=0, theta_skipped=0)
    g = {c: got_table[:, i] for i, c in enumerate(COLS)}
    t, bnd = st['table'], st['bound']
    assert np.array_equal(got_bbox, st['bbox']), what
    assert np.array_equal(got_flags, st['flags']), (what, np.flatnonzero(got_flags != st['flags'])[:10])
    for c in ('npix', 'xpeak', 'ypeak', 'peak'):
        assert np.array_equal(g[c], t[c]), (what, c)
    pos = t['flux'] > 0
    for c in ('x', 'y', 'x2', 'y2', 'xy', 'a', 'b', 'theta'):
        assert np.all(np.isnan(g[c][~pos])), (what, c, 'must be NaN where flux <= 0')
    skip = np.zeros(n, bool)
    with np.errstate(all='ignore'):
        skip[pos] = ~(((t['a'] - t['b']) / t['a'])[pos] >= THETA_CUT)        # a = b = 0 (one pixel) counts too
    skip |= ~pos
    nskip = int((skip & pos).sum())
    assert nskip <= THETA_SKIP_CAP * n, "%s: theta undefined for %d of %d sources" % (what, nskip, n)
    worst = {}
    for c in ('flux', 'x', 'y', 'x2', 'y2', 'xy', 'a', 'b', 'theta'):
        m = (~skip) if c == 'theta' else (pos if c != 'flux' else np.ones(n, bool))
        d = np.abs(g[c][m] - t[c][m])
        if c == 'theta':
            d = np.minimum(d, 180.0 - d)                 # +-90 degrees is one direction
        with np.errstate(all='ignore'):
            r = d / bnd[c][m]
        worst[c] = (float(d.max(initial=0.0)), float(np.nanmax(r, initial=0.0)))
        bad = ~(d <= bnd[c][m])
        assert not bad.any(), "%s: %s off by %g at source %d, bound %g" % (
            what, c, d[bad][0], np.flatnonzero(m)[bad][0], bnd[c][m][bad][0])
    if verbose:
        print('%s: %d sources, theta skipped for %d; max |delta| (share of bound): %s' % (
            what, n, nskip, ', '.join('%s %.1e (%.2f)' % (c, v[0], v[1]) for c, v in worst.items())))
    return dict(n=n, theta_skipped=nskip, worst=worst)
