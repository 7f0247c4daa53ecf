"""The CPU statement of the per-source error measurements (spx_measure_errors_*, csrc/spx_error_kernels.h) that
tests/test_errors_cpu.py and tests/test_gpu_errors.py compare against: numpy in float64 (np.bincount for the
sums and counts), and the checks with their derived bounds.  Not a test module itself.

Both sides start from bit-identical inputs: the frame, the label image, the rms and the TABLE the measure kernel
wrote, whose flux, x, y and peak the error kernel reads."""
import numpy as np

COLS = ('fluxerr', 'errx2', 'erry2', 'errxy', 'nhalf', 'fwhm')
FLAG_HALFMAX, FLAG_NOISE = 32, 64
U = 2.0 ** -52
T_FLUX, T_X, T_Y, T_PEAK = 1, 2, 3, 10           # columns of the measure table


def bboxes(labels, n):
    """the table of spx_label_bboxes_i32: [n + 1][4] = (xmin, ymin, xmax, ymax), row = label"""
    boxes = np.tile(np.array([2 ** 31 - 1, 2 ** 31 - 1, -1, -1], np.int32), (n + 1, 1))
    ys, xs = np.nonzero((labels > 0) & (labels <= n))
    l = labels[ys, xs]
    for col, fn, v in ((0, np.minimum, xs), (1, np.minimum, ys), (2, np.maximum, xs), (3, np.maximum, ys)):
        a = boxes[:, col].copy()
        fn.at(a, l, v.astype(np.int32))
        boxes[:, col] = a
    return boxes


def statement(frame, labels, n, table, rms, bkg=0.0, gain=None, mask=None):
    """frame [ny, nx] in its dtype; labels int32; table float64 [n, 13] as the measure kernel wrote it; rms and
    bkg scalars or frames IN THE FRAME'S DTYPE (widened to float64 here, as the kernel widens them)."""
    frame = np.asarray(frame)
    ny, nx = frame.shape
    v = frame.astype(np.float64)
    ok = np.isfinite(v) & (labels > 0) & (labels <= n)
    if mask is not None:
        ok &= ~np.asarray(mask, bool)
    ys, xs = np.nonzero(ok)
    l = labels[ys, xs] - 1
    flux, cx, cy, peak = (np.asarray(table, np.float64).reshape(n, 13)[:, c] for c in (T_FLUX, T_X, T_Y, T_PEAK))

    def at(a):
        a = np.asarray(a)
        return a.astype(np.float64)[ys, xs] if a.ndim else np.full(len(ys), float(a))
    with np.errstate(all='ignore'):
        w = v[ys, xs] - at(bkg)
        sg = at(rms)
        badsg = ~np.isfinite(sg) | (sg < 0)
        sg = np.where(badsg, 0.0, sg)
        use_gain = gain is not None and gain > 0 and np.isfinite(gain)
        shot = np.where(w > 0, w / gain, 0.0) if use_gain else np.zeros(len(w))
        v2 = sg * sg + shot
        ux, uy = xs.astype(np.float64) - cx[l], ys.astype(np.float64) - cy[l]
        terms = [v2, v2 * (ux * ux), v2 * (uy * uy), v2 * (ux * uy)]
        S = [np.bincount(l, weights=t, minlength=n) for t in terms]
        A = [np.bincount(l, weights=np.abs(t), minlength=n) for t in terms]
        npix = np.bincount(l, minlength=n)
        pos = (flux > 0) & np.isfinite(flux)
        haspeak = peak > 0
        nhalf = np.bincount(l, weights=(haspeak[l] & (w >= 0.5 * peak[l])), minlength=n).astype(np.int64)
        noise = np.bincount(l, weights=badsg, minlength=n) > 0
        f2 = flux * flux
        fluxerr = np.sqrt(S[0])
        err = [np.where(pos, S[k] / f2, np.nan) for k in (1, 2, 3)]
        fwhm = np.where(haspeak, 2.0 * np.sqrt(nhalf.astype(np.float64) / 3.14159265358979323846), np.nan)
        # ---- bounds.  A term is the same chain of IEEE operations on the same float64 inputs on both sides; were
        # it not, its roundings -- three in v2 (s s, w / gain, +), two in u u (the subtraction counts twice in a
        # square), two products -- are at most 8 * 2^-53 of the term on each side: 8 U sum|term|.  The sums add npix
        # terms in float64 in SOME order on each side, each within (npix - 1) 2^-53 sum|term| of the exact sum:
        # |delta S| <= (npix + 8) U sum|term|.
        bS = [(npix + 8) * U * a for a in A]
        # sqrt: |sqrt s - sqrt s'| <= |s - s'| / sqrt(s) and <= sqrt|s - s'|; its own rounding on both sides, 4 U
        tiny = np.finfo(np.float64).tiny
        bfe = bS[0] / np.maximum(np.maximum(fluxerr, np.sqrt(bS[0])), tiny) + 4 * U * fluxerr
        # S / (flux flux): flux is the same number on both sides, so only the sum's delta and the roundings of the
        # product and the quotient on each side: 4 U
        berr = [bS[k] / f2 + 4 * U * np.abs(S[k] / f2) for k in (1, 2, 3)]
    flags = (FLAG_HALFMAX * ((npix > 0) & (nhalf == npix)) | FLAG_NOISE * noise).astype(np.int32)
    tab = dict(fluxerr=fluxerr, errx2=err[0], erry2=err[1], errxy=err[2], nhalf=nhalf.astype(np.float64), fwhm=fwhm)
    bound = dict(fluxerr=bfe, errx2=berr[0], erry2=berr[1], errxy=berr[2])
    return dict(n=n, table=tab, bound=bound, flags=flags, npix=npix, pos=pos, haspeak=haspeak)


def check(got, got_flags, st, what='', verbose=True):
    """got float64 [n, 6] in COLS order, got_flags int32 [n].  nhalf, fwhm, the flags and the NaN pattern: exact
    (fwhm to the bit).  The four sums: the bounds above."""
    n = st['n']
    got, got_flags = np.asarray(got), np.asarray(got_flags)
    assert got.shape == (n, len(COLS)) and got_flags.shape == (n,), (what, got.shape, got_flags.shape)
    if n == 0:
        return dict(n=0)
    g = {c: got[:, i] for i, c in enumerate(COLS)}
    t, bnd = st['table'], st['bound']
    assert np.array_equal(got_flags, st['flags']), (what, np.flatnonzero(got_flags != st['flags'])[:10])
    assert np.array_equal(g['nhalf'], t['nhalf']), (what, 'nhalf')
    hp = st['haspeak']
    assert np.array_equal(np.isnan(g['fwhm']), ~hp), (what, 'fwhm NaN pattern')
    assert g['fwhm'][hp].tobytes() == t['fwhm'][hp].tobytes(), (what, 'fwhm differs in its bits')
    assert not np.isnan(g['fluxerr']).any(), (what, 'fluxerr is never NaN')
    worst = {}
    for c in ('fluxerr', 'errx2', 'erry2', 'errxy'):
        m = np.ones(n, bool) if c == 'fluxerr' else st['pos']
        assert np.all(np.isnan(g[c][~m])), (what, c, 'must be NaN where flux is not > 0')
        assert not np.isnan(g[c][m]).any(), (what, c, 'NaN where flux > 0')
        d = np.abs(g[c][m] - t[c][m])
        with np.errstate(all='ignore'):
            r = d / bnd[c][m]
        worst[c] = (float(d.max(initial=0.0)), float(np.nanmax(r, initial=0.0)))
        bad = ~(d <= bnd[c][m])
        assert not bad.any(), "%s: %s off by %g at source %d, bound %g" % (
            what, c, d[bad][0], np.flatnonzero(m)[bad][0], bnd[c][m][bad][0])
    if verbose:
        print('%s: %d sources (%d with flux > 0, %d with a peak > 0), flags %s; max |delta| (share of bound): %s' % (
            what, n, st['pos'].sum(), st['haspeak'].sum(), sorted(set(st['flags'].tolist())),
            ', '.join('%s %.1e (%.2f)' % (c, x[0], x[1]) for c, x in worst.items())))
    return dict(n=n, worst=worst)
