"""Steps 2' (combine_type='minmed', combine_grow) and 7 (driz_cr_grow, driz_cr_ctegrow) of include/subpixal_hip.h stated
a second time in numpy, independently of the kernels (spx_minmed_kernels.h).  Not a test module.

The definitions are the library's own, modelled on drizzlepac's; drizzlepac is not in the reference tree, so parity
with it is UNPINNED.  Every decision is float64 arithmetic made of + - * / and comparisons (no sqrt), which numpy
evaluates exactly as the kernels do (contraction off): the tests compare with EXACT equality, no bound is needed.

Step 1 (the single-frame values `vals` float32 [K][NY][NX], `valid` bool) is an input, as in crreject_statement.py.

STEP 2'.  For output pixel P with m valid s_k:
    md = step 2's median (nlow / nhigh as given);  lo = the smallest valid s_k;  kmin = the lowest row that has it;
    var = r^2 + (g > 0 ? max(lo - sky, 0) / g : 0) with (r, sky, g) = table[kmin];  t = md - lo;
    hit_p = m >= 2 and t > 0 and t t > (n_p n_p) var;  seed = hit_1;
    use_min = seed or (hit_2 and a seed within Chebyshev distance grow, inside the grid);
    med = use_min ? lo : md;  minmed = 0 median, 1 own test, 2 neighbour rule.
STEP 7.  Seeds = step 6's crmask.  A non-seed is flagged iff it is testable (inside the frame, finite, unmasked,
    weight > 0, valid rms, b defined) and a seed lies in the g x g block centred on it or at (i, j - ctedir tau),
    tau = 1 .. c.  Row index j, column index i: the tail runs along columns."""
import numpy as np

import crreject_statement as cs

DEFAULTS = dict(nsigma=(4.0, 3.0), grow=1)


def _shift(a, dy, dx):
    """out[y, x] = a[y + dy, x + dx], False outside (any shift, also one longer than the array)"""
    ny, nx = a.shape
    out = np.zeros(a.shape, bool)
    if abs(dy) < ny and abs(dx) < nx:
        out[max(-dy, 0):ny - max(dy, 0), max(-dx, 0):nx - max(dx, 0)] = \
            a[max(dy, 0):ny - max(-dy, 0), max(dx, 0):nx - max(-dx, 0)]
    return out


def dilate(seed, half):
    """a seed within Chebyshev distance `half`, inside the grid"""
    out = np.zeros(seed.shape, bool)
    for dy in range(-half, half + 1):
        for dx in range(-half, half + 1):
            out |= _shift(seed, dy, dx)
    return out


def table_of(c):
    """float64 [K][3] = (combine_rms, sky, gain or 0) of a case: `combine_rms` where it has one, else its scalar rms"""
    p = dict(cs.DEFAULTS)
    p.update(c.get('cr', {}))
    g = p['gain']
    g = float(g) if g is not None and np.isfinite(g) and g > 0 else 0.0
    rms = c.get('combine_rms') or c['rms']
    return np.array([[float(r), float(p['sky']), g] for r in rms], np.float64)


def minmed(vals, valid, table, nsigma=(4.0, 3.0), grow=1, nlow=0, nhigh=0):
    """dict(md, lo, kmin, hit (two planes), med, nmed, minmed) of step 2'"""
    K, NY, NX = vals.shape
    md, nmed = cs.median(vals, valid, nlow, nhigh)
    m = valid.sum(axis=0)
    stack = np.where(valid, vals.astype(np.float32), np.float32(np.inf))
    kmin = np.argmin(stack, axis=0)                                  # the first occurrence: the lowest row
    lo = np.take_along_axis(stack, kmin[None], axis=0)[0]
    lo = np.where(m > 0, lo, np.float32(0)).astype(np.float32)
    kmin = np.where(m > 0, kmin, 0)
    table = np.asarray(table, np.float64)
    r, sky, g = table[kmin, 0], table[kmin, 1], table[kmin, 2]
    lo64 = lo.astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        var = r * r + np.where(g > 0, np.maximum(lo64 - sky, 0.0) / np.where(g > 0, g, 1.0), 0.0)
    t = md.astype(np.float64) - lo64
    hit = [(m >= 2) & (t > 0) & (t * t > (float(n) * float(n)) * var) for n in nsigma]
    seed = hit[0]
    near = dilate(seed, int(grow)) if grow else np.zeros_like(seed)
    how = np.where(seed, 1, np.where(hit[1] & near, 2, 0)).astype(np.uint8)
    med = np.where(how > 0, lo, md).astype(np.float32)
    return dict(md=md, lo=lo, kmin=kmin, hit=hit, med=med, nmed=nmed, minmed=how)


def defined(m, nmed, ny, nx):
    """step 3's DEFINED flag on the frame, from integer decisions alone: the position inside the grid and nmed > 0 on
    the quintic's clipped footprint (a summed-area table of nmed == 0)"""
    NY, NX = nmed.shape
    a0, a1, a2, a3, a4, a5 = [float(v) for v in m]
    j, i = np.mgrid[0:ny, 0:nx].astype(np.float64)
    X, Y = (a0 * i + a1 * j) + a2, (a3 * i + a4 * j) + a5
    ok = (X >= 0.0) & (X <= NX - 1) & (Y >= 0.0) & (Y <= NY - 1)
    ix, iy = np.where(ok, X, 0.0).astype(np.int64), np.where(ok, Y, 0.0).astype(np.int64)
    sat = np.zeros((NY + 1, NX + 1), np.int64)
    sat[1:, 1:] = np.cumsum(np.cumsum(nmed == 0, axis=0), axis=1)
    xa, xb = np.maximum(ix - 2, 0), np.minimum(ix + 3, NX - 1) + 1
    ya, yb = np.maximum(iy - 2, 0), np.minimum(iy + 3, NY - 1) + 1
    empty = sat[yb, xb] - sat[ya, xb] - sat[yb, xa] + sat[ya, xa]
    return ok & (empty == 0)


def testable(d, weight, mask, m, nmed, rms):
    """step 5's TESTABLE"""
    d = np.asarray(d, np.float64)
    r = np.broadcast_to(np.asarray(rms, np.float64), d.shape)
    ok = np.isfinite(d) & np.isfinite(r) & (r >= 0) & defined(m, nmed, *d.shape)
    if mask is not None:
        ok &= np.asarray(mask) == 0
    if weight is not None:
        w = np.asarray(weight, np.float64)
        ok &= np.isfinite(w) & (w > 0)
    return ok


def grow_mask(seed, ok, g=1, c=0, ctedir=0):
    """step 7: the grown mask (bool) of a seed mask and the testable plane"""
    seed = np.asarray(seed) != 0
    reach = dilate(seed, (int(g) - 1) // 2)
    if ctedir:
        for tau in range(1, int(c) + 1):
            reach |= _shift(seed, -int(ctedir) * tau, 0)              # a seed at (i, j - ctedir tau)
    return seed | (reach & ok)


def reject(vals, valid, c, combine_type='median', nsigma=(4.0, 3.0), grow=1):
    """steps 2 / 2' .. 6 of a case from its single-frame values, by the statement alone: (combined image, nmed, per
    frame crreject_statement.frame_cr's dict or None)"""
    p = dict(cs.DEFAULTS)
    p.update(c.get('cr', {}))
    K = len(c['frames'])
    act = [True] * K if c['active'] is None else [bool(a) for a in c['active']]
    vv = valid & np.array(act)[:, None, None]
    if combine_type == 'minmed':
        st = minmed(vals, vv, table_of(c), nsigma, grow, p['nlow'], p['nhigh'])
        med, nmed = st['med'], st['nmed']
    else:
        med, nmed = cs.median(vals, vv, p['nlow'], p['nhigh'])
    frames = [None if not act[k] else
              cs.frame_cr(c['frames'][k], None if c['weights'] is None else c['weights'][k],
                          None if c['masks'] is None else c['masks'][k], c['maps'][k], med, nmed, c['rms'][k],
                          sky=p['sky'], gain=p['gain'], snr=p['snr'], scale=p['scale']) for k in range(K)]
    return med, nmed, frames
