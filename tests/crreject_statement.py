"""The cosmic-ray rejection of include/subpixal_hip.h stated a second time in numpy, independently of the kernels
(spx_crreject_kernels.h).  Not a test module.

STEP 1 is the drizzle's own arithmetic and has its statement already (tests/drizzle_statement.py, a scatter): this
module takes the single-frame values `vals` float32 [K][NY][NX] and `valid` bool [K][NY][NX] as INPUT.  The tests get
them from K runs of the existing drizzle with one frame active each (bit for bit what item 1 defines), so that `med`
and `nmed` can be compared exactly; `singles_by_scatter` makes them from the scatter for the tests that look at the
statement alone (they differ from the kernel's by a float32 rounding at most, which changes no statistics).

STEPS 2 .. 6 are restated here: the median by np.sort; the blot as the float64 Lagrange form of the oracle
(oracle/subpixal_oracle.py: _lagrange6, _continued), which is what the kernel's float32 Everett form is pinned
against (tests/blot_cases.py); the derivative, the two tests and the neighbour rule in float64.

BOUNDS.  u = 2^-24.  P = max |continued 6 x 6 patch| of med around the blot position.
  the blot.  tests/blot_cases.py pins |b_kernel - b_exact| <= C u P with C = 5.05, at positions whose fractional parts
    are dyadic.  Here they are not: the kernel rounds the fractions (sx, sy) to float32, an error of at most u / 2
    each, and the position itself carries 4 roundings of float64 numbers below Cmax = 64 (negligible: 2^-45).  The
    interpolant is sum_ij w_i(sy) w_j(sx) c_ij, so moving sx by e changes it by at most e L' L P with
    L = max_s sum |w_i(s)| and L' = max_s sum |w_i'(s)| (computed below from the same weights: 1.39 and 2.54, so C + L' L = 8.58):
        Bb = (C + L' L) u P + 2^-40 P
  the derivative.  D = max_n |b - b_n| over the same set of neighbours (the defined-flags are integer decisions):
        BD = Bb + max_n Bb(n) + u D        (the float32 subtraction rounds once)
  a test.  t = |d - b| moves by Bb; thr_p = scale_p D + snr_p sqrt(var), var = rms^2 + max(b - sky, 0) / gain, and
    |sqrt(v) - sqrt(v')| = |v - v'| / (sqrt(v) + sqrt(v')) <= (Bb / gain) / sqrt(v) (sqrt(Bb / gain) where v = 0);
    the float64 chain itself adds fewer than 16 roundings of numbers no larger than t + thr:
        Bm_p = Bb + scale_p BD + snr_p dsqrt + 16 * 2^-53 (t + thr_p)
  A pixel's DECISION is safe when |t - thr_2| > Bm_2 there and, if it fails test 2, |t - thr_1| > Bm_1 on every
  testable pixel of its 3 x 3 block; implementations must agree with `crmask` on every safe pixel.  The bound is
  derived from the pinned blot error and the operation chain, not from what any kernel gives.
"""
import numpy as np

from oracle import subpixal_oracle as orc

import drizzle_statement as ds

U = 2.0 ** -24
BLOT_C = 5.05                     # tests/blot_cases.py: C
_S = np.linspace(0.0, 1.0, 2001)
_W = np.array([orc._lagrange6(s) for s in _S])
LEBESGUE = float(np.abs(_W).sum(axis=1).max())
# the weights are quintics: a central difference over h = 1e-4 is off by h^2 / 6 |w'''| < 1e-7
DERIV = float(max(np.abs((orc._lagrange6(s + 1e-4) - orc._lagrange6(s - 1e-4)) / 2e-4).sum() for s in _S)) * 1.001
BLOT_K = BLOT_C + DERIV * LEBESGUE
DEFAULTS = dict(snr=(3.5, 3.0), scale=(1.2, 0.7), nlow=0, nhigh=0, sky=0.0, gain=None)


def singles_by_scatter(c):
    """the single-frame drizzles of every frame of case `c` from the scatter of drizzle_statement (inactive frames:
    nothing valid)"""
    K = len(c['frames'])
    NY, NX = c['out_shape']
    vals = np.zeros((K, NY, NX), np.float32)
    valid = np.zeros((K, NY, NX), bool)
    for k in range(K):
        if c['active'] is not None and not c['active'][k]:
            continue
        st = ds.statement([c['frames'][k]], [c['maps'][k]], c['out_shape'],
                          weights=None if c['weights'] is None else [c['weights'][k]],
                          masks=None if c['masks'] is None else [c['masks'][k]],
                          pixfrac=c['pixfrac'], kernel=c['kernel'])
        valid[k] = st['wht'] > 0
        vals[k] = np.where(valid[k], st['sci'], 0.0).astype(np.float32)
    return vals, valid


def median(vals, valid, nlow=0, nhigh=0):
    K, NY, NX = vals.shape
    med = np.zeros((NY, NX), np.float32)
    nmed = valid.sum(axis=0).astype(np.uint8)
    for Y in range(NY):
        for X in range(NX):
            v = np.sort(vals[valid[:, Y, X], Y, X].astype(np.float32))
            m = len(v)
            if m == 0:
                continue
            if m - nlow - nhigh >= 1:
                v = v[nlow:m - nhigh]
            n = len(v)
            med[Y, X] = v[n // 2] if n % 2 else np.float32(0.5 * (float(v[n // 2 - 1]) + float(v[n // 2])))
    return med, nmed


def blot(med, nmed, m, ny, nx, halo=1):
    """b, its defined-flag and Bb on the frame grown by `halo`: index [j + halo][i + halo]"""
    NY, NX = med.shape
    m64 = med.astype(np.float64)
    ext = np.array([[orc._continued(m64, j, i) for i in range(-2, NX + 3)] for j in range(-2, NY + 3)])
    a0, a1, a2, a3, a4, a5 = [float(v) for v in m]
    shape = (ny + 2 * halo, nx + 2 * halo)
    b, bound, defined = np.zeros(shape), np.zeros(shape), np.zeros(shape, bool)
    for j in range(-halo, ny + halo):
        for i in range(-halo, nx + halo):
            X, Y = (a0 * i + a1 * j) + a2, (a3 * i + a4 * j) + a5
            if not (0.0 <= X <= NX - 1 and 0.0 <= Y <= NY - 1):
                continue
            ix, iy = int(np.floor(X)), int(np.floor(Y))
            if not nmed[max(iy - 2, 0):min(iy + 3, NY - 1) + 1, max(ix - 2, 0):min(ix + 3, NX - 1) + 1].all():
                continue
            patch = ext[iy:iy + 6, ix:ix + 6]
            defined[j + halo, i + halo] = True
            b[j + halo, i + halo] = orc._lagrange6(Y - iy) @ patch @ orc._lagrange6(X - ix)
            bound[j + halo, i + halo] = (BLOT_K * U + 2.0 ** -40) * np.abs(patch).max()
    return b, defined, bound


def _shifted(a, dy, dx, fill):
    out = np.full(a.shape, fill, a.dtype)
    ny, nx = a.shape
    out[max(-dy, 0):ny - max(dy, 0), max(-dx, 0):nx - max(dx, 0)] = a[max(dy, 0):ny - max(-dy, 0), max(dx, 0):nx - max(-dx, 0)]
    return out


def frame_cr(d, weight, mask, m, med, nmed, rms, sky=0.0, gain=None, snr=(3.5, 3.0), scale=(1.2, 0.7)):
    """steps 3 .. 6 for one frame: dict(b, defined, bb, D, testable, t, thr, fail, margin_ok, crmask, safe)"""
    d = np.asarray(d, np.float64)
    ny, nx = d.shape
    bh, defh, bbh = blot(med, nmed, m, ny, nx, halo=2)
    # the derivative on the frame grown by 1 (so that out-of-frame neighbours of edge pixels are there)
    core = (slice(1, -1), slice(1, -1))
    D = np.zeros((ny + 2, nx + 2))
    BDn = np.zeros((ny + 2, nx + 2))
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        nb, nd, nbb = _shifted(bh, dy, dx, 0.0)[core], _shifted(defh, dy, dx, False)[core], _shifted(bbh, dy, dx, 0.0)[core]
        diff = np.abs((bh[core].astype(np.float32) - nb.astype(np.float32)).astype(np.float64))
        D = np.where(nd, np.maximum(D, diff), D)
        BDn = np.where(nd, np.maximum(BDn, nbb), BDn)
    inner = (slice(1, -1), slice(1, -1))
    b, defined, bb = bh[core][inner], defh[core][inner], bbh[core][inner]
    D, BDn = D[inner], BDn[inner]
    BD = bb + BDn + U * D
    r = np.broadcast_to(np.asarray(rms, np.float64), d.shape)
    testable = np.isfinite(d) & defined & np.isfinite(r) & (r >= 0)
    if mask is not None:
        testable &= np.asarray(mask) == 0
    if weight is not None:
        w = np.asarray(weight, np.float64)
        testable &= np.isfinite(w) & (w > 0)
    g = float(gain) if gain is not None and np.isfinite(gain) and gain > 0 else 0.0
    with np.errstate(invalid='ignore'):
        t = np.abs(d - b)
        var = np.where(testable, r, 0.0) ** 2
        if g:
            var = var + np.maximum(b - float(sky), 0.0) / g
        sq = np.sqrt(var)
        with np.errstate(divide='ignore'):
            dsq = np.where(var > 0, (bb / g) / np.where(var > 0, sq, 1.0), np.sqrt(bb / g)) if g else np.zeros_like(bb)
        thr, fail, ok = [], [], []
        for p in range(2):
            th = scale[p] * D + snr[p] * sq
            bm = bb + scale[p] * BD + snr[p] * dsq + 16.0 * ds.EPS * (np.where(testable, t, 0.0) + th)
            thr.append(th)
            fail.append(testable & (t > th))
            ok.append(~testable | (np.abs(np.where(testable, t, 0.0) - th) > bm))
    any1 = np.zeros(d.shape, bool)
    ok1 = np.ones(d.shape, bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            any1 |= _shifted(fail[0], dy, dx, False)
            ok1 &= _shifted(ok[0], dy, dx, True)
    crmask = fail[1] & any1
    safe = ok[1] & (~fail[1] | ok1)
    return dict(b=b, defined=defined, bb=bb, D=D, testable=testable, t=t, thr=thr, fail=fail, crmask=crmask, safe=safe)


def statement(c, vals, valid):
    """the whole of a case of crreject_cases.py from its single-frame values: med, nmed and, per frame (None for an
    inactive one), frame_cr's dict"""
    p = dict(DEFAULTS)
    p.update(c.get('cr', {}))
    K = len(c['frames'])
    act = [True] * K if c['active'] is None else [bool(a) for a in c['active']]
    vv = valid & np.array(act)[:, None, None]
    med, nmed = median(vals, vv, p['nlow'], p['nhigh'])
    frames = []
    for k in range(K):
        if not act[k]:
            frames.append(None)
            continue
        frames.append(frame_cr(c['frames'][k], None if c['weights'] is None else c['weights'][k],
                               None if c['masks'] is None else c['masks'][k], c['maps'][k], med, nmed,
                               c['rms'][k], sky=p['sky'], gain=p['gain'], snr=p['snr'], scale=p['scale']))
    return dict(med=med, nmed=nmed, frames=frames, params=p)


def check_frame(crmask, clean, d, st, dtype, what=''):
    """an implementation's crmask and clean of one frame against frame_cr's dict: the mask on every safe pixel, never
    outside testable; clean == d bit for bit off the mask, and b within the blot bound (plus the cast) on it"""
    d = np.asarray(d, dtype)
    assert crmask.dtype == np.uint8 and crmask.shape == d.shape and clean.dtype == np.dtype(dtype), what
    assert set(np.unique(crmask)) <= {0, 1}, what
    got = crmask.astype(bool)
    assert not (got & ~st['testable']).any(), '%s: flagged pixels that are not testable' % what
    bad = (got != st['crmask']) & st['safe']
    assert not bad.any(), '%s: crmask differs on %d safe pixels' % (what, int(bad.sum()))
    assert clean[~got].tobytes() == d[~got].tobytes(), '%s: clean differs from the frame off the mask' % what
    u = U if np.dtype(dtype) == np.float32 else ds.EPS
    err = np.abs(clean[got].astype(np.float64) - st['b'][got])
    lim = st['bb'][got] + u * np.abs(st['b'][got])
    assert np.all(err <= lim), '%s: clean off the blot by %g (bound %g)' % (what, err.max(), lim[np.argmax(err - lim)])
    return int((~st['safe'] & st['testable']).sum())
