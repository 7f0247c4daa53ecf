"""The CPU statement of background estimation that tests/test_background_cpu.py and tests/test_gpu_background.py
compare against: numpy/scipy in float64, independent of the code under test (np.sort, np.median, np.mean / np.std,
scipy.interpolate.CubicSpline), and the checks with their derived bounds.  Not a test module itself.

Definitions: include/subpixal_hip.h (background block).  Two decisions rest on comparisons that rounding could
flip, the clip edges med +- kappa std and the branch |mean - med| < 0.3 std: a value (or |mean - med|) within the
derived rounding of such an edge is a TIE, and a scene with a tie is a test-construction error (rebuild it with
another seed), not a failure of the code under test.

BOUNDS (U = 2^-52)
  mean: both sides add m terms in float64 in some order, each sum within (m - 1) 2^-53 sum|v| of the exact one, so
      the two sums differ by less than m U sum|v| ... / m for the means:  bmean = U sum|v| + 4 U |mean|  (the
      division and the conversion round once more on each side).
  std: with d = v - mean, each side's d carries the shift of its mean (<= bmean) and one rounding U |d|; sum|d| <=
      m std.  |d var| <= 2 std bmean + bmean^2 + (m + 8) U var, and |d sqrt(var)| <= |d var| / std:
      bstd = (2 std bmean + bmean^2 + (m + 8) U var) / std + 4 U std.
  clip edge med +- kappa std: bedge = kappa bstd + 4 U (|med| + kappa std).
  branch: ||mean - med| - 0.3 std| against bmean + 0.3 bstd + 4 U (|mean| + |med| + std).
  cell bkg: mean -> bmean; med -> 0 (a selection, or one exact-to-rounding average on identical inputs);
      2.5 med - 1.5 mean -> 1.5 bmean + 4 U (2.5 |med| + 1.5 |mean|).
  filtered mesh: a median moves by at most the largest move of its inputs: max of the good cells' bounds
      + 2 U max|node|.
  maps: the spline's scaled second derivatives m = M h^2 / 6 solve (1 4 1) m = (1 -2 1) z, so
      max|m| <= (1 / (4 - 2)) 4 max|z| = 2 max|z|; a value is A z0 + B z1 + (A^3 - A) m0 + (B^3 - B) m1 with
      A + B = 1 and |A^3 - A| + |B^3 - B| <= 3/4: at most 2.5 max|z| per axis, K = 6.25 for both.  A node error e
      therefore moves a map by at most K e; the float64 arithmetic of either side (some 20 operations on
      quantities of at most K max|node|, 4 U each allowed) by 64 U K max|node|; the one rounding to the maps'
      dtype by eps(dtype) |value|:   bmap = K (bnode + 64 U max|node|) + eps(dtype) (|value| + that).
  threshold: bmap_bkg + nsigma bmap_rms + eps(float32) |thr| (and the same rounding of its two inputs is inside
      bmap already).
"""
import math

import numpy as np
from scipy.interpolate import CubicSpline

U = 2.0 ** -52
K_SPLINE = 6.25


class SceneTie(AssertionError):
    """the scene has a decision within rounding: rebuild it"""


class NoGoodCell(Exception):
    pass


def cell_statistics(v, kappa, max_iters):
    """v: the usable values of one cell, any order.  Returns dict(lo, hi, med, mean, std, rounds, bounds, ties)."""
    s = np.sort(np.asarray(v, np.float64))
    lo, hi = 0, len(s)
    ties = 0
    rounds = 0
    history = []
    while True:
        r = s[lo:hi]
        m = hi - lo
        med = float(np.median(r))
        if r[0] == r[-1]:
            mean, std, bmean, bstd = float(r[0]), 0.0, 0.0, 0.0
            history.append((lo, hi))
            break
        mean, std = float(np.mean(r)), float(np.std(r))
        bmean = U * float(np.abs(r).sum()) + 4 * U * abs(mean)
        var = std * std
        assert std > 0.0
        bstd = (2 * std * bmean + bmean ** 2 + (m + 8) * U * var) / std + 4 * U * std
        if std <= bstd:
            ties += 1
        history.append((lo, hi))
        if rounds >= max_iters:
            break
        lower, upper = med - kappa * std, med + kappa * std
        bedge = kappa * bstd + 4 * U * (abs(med) + kappa * std)
        ties += int(np.sum(np.abs(r - lower) <= bedge) + np.sum(np.abs(r - upper) <= bedge))
        keep = np.flatnonzero((r >= lower) & (r <= upper))
        if len(keep) == 0:
            break
        nlo, nhi = lo + int(keep[0]), lo + int(keep[-1]) + 1
        assert nhi - nlo == len(keep)
        if (nlo, nhi) == (lo, hi):
            break
        lo, hi = nlo, nhi
        rounds += 1
    if std == 0.0:
        bkg, bbkg, branch = mean, bmean, 'mean'
    else:
        gap = abs(mean - med)
        if abs(gap - 0.3 * std) <= bmean + 0.3 * bstd + 4 * U * (abs(mean) + abs(med) + std):
            ties += 1
        if gap < 0.3 * std:
            bkg, branch = 2.5 * med - 1.5 * mean, 'mode'
            bbkg = 1.5 * bmean + 4 * U * (2.5 * abs(med) + 1.5 * abs(mean))
        else:
            bkg, bbkg, branch = med, 0.0, 'med'
    return dict(lo=lo, hi=hi, med=med, mean=mean, std=std, bkg=bkg, rounds=rounds, history=history, branch=branch,
                bmean=bmean, bstd=bstd, bbkg=bbkg, ties=ties)


def mesh(frame, box, mask=None, exclude=None, kappa=3.0, max_iters=10, min_good_fraction=0.5):
    f = np.asarray(frame)
    ny, nx = f.shape
    bh, bw = box
    ncy, ncx = -(-ny // bh), -(-nx // bw)
    ok = np.isfinite(f)
    if mask is not None:
        ok &= ~np.asarray(mask, bool)
    if exclude is not None:
        ok &= np.asarray(exclude) == 0
    v64 = f.astype(np.float64)
    mb = np.full((ncy, ncx), np.nan)
    mr = np.full((ncy, ncx), np.nan)
    bb = np.zeros((ncy, ncx))
    br = np.zeros((ncy, ncx))
    ng = np.zeros((ncy, ncx), np.int32)
    good = np.zeros((ncy, ncx), bool)
    cells = {}
    ties = 0
    for j in range(ncy):
        for i in range(ncx):
            sl = (slice(j * bh, min(ny, (j + 1) * bh)), slice(i * bw, min(nx, (i + 1) * bw)))
            vals = v64[sl][ok[sl]]
            n = len(vals)
            ng[j, i] = n
            need = max(2, math.ceil(min_good_fraction * ok[sl].size))
            if n == 0:
                continue
            c = cell_statistics(vals, kappa, max_iters)
            cells[(j, i)] = c
            ties += c['ties']
            if n >= need:
                good[j, i] = True
                mb[j, i], mr[j, i], bb[j, i], br[j, i] = c['bkg'], c['std'], c['bbkg'], c['bstd']
    return dict(bkg=mb, rms=mr, ngood=ng, good=good, bbkg=bb, brms=br, cells=cells, ties=ties)


def filter_mesh(z, good, fs):
    if not good.any():
        raise NoGoodCell()
    ncy, ncx = z.shape
    r = fs // 2
    glob = float(np.median(z[good]))
    out = np.empty_like(z)
    for j in range(ncy):
        for i in range(ncx):
            sl = (slice(max(0, j - r), j + r + 1), slice(max(0, i - r), i + r + 1))
            w = z[sl][good[sl]]
            out[j, i] = float(np.median(w)) if len(w) else glob
    return out


def _spline_axis(z, axis, box, npix):
    n = z.shape[axis]
    c = np.arange(n) * box + (box - 1) / 2.0
    q = np.clip(np.arange(npix, dtype=np.float64), c[0], c[-1])
    if n == 1:
        return np.repeat(z, npix, axis=axis)
    return CubicSpline(c, z, axis=axis, bc_type='natural')(q)


def expand(z, shape, box):
    """tensor-product natural cubic spline: along y, then along x"""
    return _spline_axis(_spline_axis(z, 0, box[0], shape[0]), 1, box[1], shape[1])


def statement(frame, box=(64, 64), filter_size=3, mask=None, exclude=None, sigma=3.0, max_iters=10,
              min_good_fraction=0.5, nsigma=None, allow_ties=False):
    f = np.asarray(frame)
    me = mesh(f, box, mask, exclude, sigma, max_iters, min_good_fraction)
    if me['ties'] and not allow_ties:
        raise SceneTie("scene has %d decisions within rounding of an edge" % me['ties'])
    fb = filter_mesh(me['bkg'], me['good'], filter_size)
    fr = filter_mesh(me['rms'], me['good'], filter_size)
    bfb = float(me['bbkg'][me['good']].max()) + 2 * U * float(np.abs(fb).max())
    bfr = float(me['brms'][me['good']].max()) + 2 * U * float(np.abs(fr).max())
    eps = float(np.finfo(f.dtype if f.dtype == np.float64 else np.float32).eps)
    bkg = expand(fb, f.shape, box)
    rms = np.maximum(expand(fr, f.shape, box), 0.0)
    nb = K_SPLINE * (bfb + 64 * U * float(np.abs(fb).max()))
    nr = K_SPLINE * (bfr + 64 * U * float(np.abs(fr).max()))
    bmap_b = nb + eps * (np.abs(bkg) + nb)
    bmap_r = nr + eps * (np.abs(rms) + nr)
    out = dict(mesh=me, filt_bkg=fb, filt_rms=fr, bfilt_bkg=bfb, bfilt_rms=bfr, bkg=bkg, rms=rms, bmap_bkg=bmap_b,
               bmap_rms=bmap_r, dtype=np.float64 if f.dtype == np.float64 else np.float32)
    if nsigma is not None:
        thr = bkg + nsigma * rms
        out['thr'] = thr
        out['bthr'] = bmap_b + abs(nsigma) * bmap_r + float(np.finfo(np.float32).eps) * (np.abs(thr) + bmap_b + abs(nsigma) * bmap_r)
    return out


def check_mesh(got_bkg, got_rms, got_ngood, st, what=''):
    """the unfiltered mesh: ngood equal, bad cells NaN, good cells within the cell bounds (med branch: bit-equal)"""
    me = st['mesh']
    assert got_ngood.shape == me['ngood'].shape, what
    assert np.array_equal(got_ngood, me['ngood']), (what, 'ngood')
    g = me['good']
    assert np.all(np.isnan(got_bkg[~g])) and np.all(np.isnan(got_rms[~g])), (what, 'bad cells must be NaN')
    db, dr = np.abs(got_bkg[g] - me['bkg'][g]), np.abs(got_rms[g] - me['rms'][g])
    assert np.all(db <= me['bbkg'][g]), (what, 'mesh bkg', float(db.max()), float(me['bbkg'][g].max()))
    assert np.all(dr <= me['brms'][g]), (what, 'mesh rms', float(dr.max()), float(me['brms'][g].max()))
    return float(db.max(initial=0.0)), float(dr.max(initial=0.0))


def check_cells(got, st, what=''):
    """got: {(j, i): (lo, hi, med, mean, std)} as the kernel left them; ranges equal, med bit-equal"""
    for key, (lo, hi, med, mean, std) in got.items():
        c = st['mesh']['cells'][key]
        assert (lo, hi) == (c['lo'], c['hi']), (what, key, (lo, hi), (c['lo'], c['hi']))
        assert med == c['med'], (what, key, 'med', med, c['med'])
        assert abs(mean - c['mean']) <= c['bmean'], (what, key, 'mean')
        assert abs(std - c['std']) <= c['bstd'], (what, key, 'std')


def check_maps(got_bkg, got_rms, got_thr, st, what='', filt=None, verbose=True):
    """maps in the frame's dtype (thr float32), each within its bound; `filt` = (filtered bkg mesh, rms mesh)"""
    worst = {}
    if filt is not None:
        for name, g, z, b in (('bkg', filt[0], st['filt_bkg'], st['bfilt_bkg']), ('rms', filt[1], st['filt_rms'], st['bfilt_rms'])):
            d = float(np.abs(g - z).max())
            assert d <= b, (what, 'filtered mesh ' + name, d, b)
    for name, g, z, b, dt in (('bkg', got_bkg, st['bkg'], st['bmap_bkg'], st['dtype']),
                              ('rms', got_rms, st['rms'], st['bmap_rms'], st['dtype']),
                              ('thr', got_thr, st.get('thr'), st.get('bthr'), np.float32)):
        if g is None:
            continue
        assert g.dtype == dt and g.shape == z.shape, (what, name, g.dtype, g.shape)
        d = np.abs(g.astype(np.float64) - z)
        bad = ~(d <= b)
        with np.errstate(all='ignore'):
            worst[name] = (float(d.max()), float(np.nanmax(d / b, initial=0.0)))
        assert not bad.any(), "%s: %s map off by %g (bound %g) at %s" % (
            what, name, d[bad].max(), b[bad].min(), np.argwhere(bad)[0])
    if got_rms is not None:
        assert np.all(got_rms >= 0), (what, 'rms must not be negative')
    if verbose:
        print('%s: max |delta| (share of bound): %s' % (what, ', '.join('%s %.1e (%.2f)' % (k, v[0], v[1])
                                                                         for k, v in worst.items())))
    return worst
