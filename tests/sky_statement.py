"""The whole-frame sigma-clipped statistics of include/subpixal_hip.h (sky block) stated a second time in numpy,
independently of the kernels: np.sort for the median, math.fsum for the two moments, the rounds as the header
numbers them.  Not a test module.

Two things in a round rest on float64 sums whose ORDER the header fixes and this statement does not follow: the
moments, and through std the new edges lo', hi'.  Per round the statement therefore computes
  * a bound on |S1 - S1'| and |S2 - S2'| from the operation chain of the kernel's sum: every term d = v - med is one
    rounding (u |d|, u = 2^-53), d * d three (the rounding of d twice, the product once), and a term passes at most
    L additions on its way into the total, L = ceil(npix / 4096) + 6 + 4 + 16 (its accumulator, the butterfly, the
    wave sums, the workgroup sums): |dS1| <= (L + 2) u sum|d|, |dS2| <= (L + 4) u sum d^2 to first order, one unit
    of each count for this statement's own fsum;
  * from these, bounds on mean, std (through var = S2 / n - (S1 / n)^2, by evaluating the square root at var +- its
    bound) and on lo' = med - lsigma std, hi' = med + usigma std, each division, product and sum adding its own
    rounding; all bounds are doubled, which covers the second-order terms;
  * the distance of the nearest usable value of the current range from each NEW edge (an edge that stays at the old
    one is exact, unless the new one lies within the bound of it).
A round is SAFE when each distance exceeds its bound and the decision std > 0 does (std > its bound); a case is safe
when every round of every frame is.  On a safe case counts, rounds and med must agree exactly with the kernels."""
import math

import numpy as np

U = 2.0 ** -53
EMPTY, BAD_FRAME = 1, 2
STATS = {'median': 0, 'mean': 1, 'mode': 2}


def usable_values(frame, weight=None, mask=None, lower=None, upper=None):
    """float64 values of the usable pixels (any order: the statement sorts)"""
    v = np.asarray(frame)
    ok = np.isfinite(v)
    if mask is not None:
        ok &= np.asarray(mask) == 0
    if weight is not None:
        w = np.asarray(weight)
        with np.errstate(invalid='ignore'):
            ok &= np.isfinite(w) & (w > 0)
    v = v.astype(np.float64)
    with np.errstate(invalid='ignore'):
        if lower is not None and lower == lower:
            ok &= v >= lower
        if upper is not None and upper == upper:
            ok &= v <= upper
    return v[ok] + 0.0                                       # -0.0 counts as +0.0


def sky_by_rule(stat, med, mean, std):
    if stat == 'median':
        return med
    if stat == 'mean':
        return mean
    if std == 0.0:
        return mean
    if abs(mean - med) < 0.3 * std:
        return 2.5 * med - 1.5 * mean
    return med


def statement(frame, weight=None, mask=None, lower=None, upper=None, lsigma=4.0, usigma=4.0, max_iters=5,
              stat='median'):
    vals = np.sort(usable_values(frame, weight, mask, lower, upper))
    npix = int(np.asarray(frame).size)
    L = -(-npix // 4096) + 6 + 4 + 16
    lo = -np.inf if lower is None or lower != lower else float(lower)
    hi = np.inf if upper is None or upper != upper else float(upper)
    res = dict(n_usable=int(vals.size), n_final=0, rounds=0, status=0, med=np.nan, mean=np.nan, std=np.nan, lo=lo,
               hi=hi, b_mean=0.0, b_std=0.0, b_lo=0.0, b_hi=0.0, safe=True, margins=[])
    if vals.size == 0:
        res['status'] = EMPTY
        res['sky'] = np.nan
        return res
    cur = vals
    b_lo = b_hi = 0.0
    for r in range(max_iters + 1):
        n = int(cur.size)
        med = float(cur[n // 2]) if n & 1 else (float(cur[(n - 1) // 2]) + float(cur[n // 2])) * 0.5
        res.update(n_final=n, rounds=r + 1, med=med, lo=lo, hi=hi, b_lo=b_lo, b_hi=b_hi)
        if cur[0] == cur[-1]:
            res.update(mean=float(cur[0]), std=0.0, b_mean=0.0, b_std=0.0)
            break
        d = cur - med
        s1, s2 = math.fsum(d), math.fsum(d * d)
        m1 = s1 / n
        mean = med + m1
        var = s2 / n - m1 * m1
        std = math.sqrt(max(var, 0.0))
        e1 = (L + 2) * U * float(np.abs(d).sum())
        e2 = (L + 4) * U * s2
        em1 = e1 / n + U * abs(m1)
        emean = 2.0 * (em1 + U * abs(mean))
        evar = e2 / n + U * s2 / n + 2.0 * abs(m1) * em1 + U * m1 * m1 + U * abs(var)
        estd = 2.0 * (max(math.sqrt(max(var + evar, 0.0)) - std, std - math.sqrt(max(var - evar, 0.0))) + U * std)
        res.update(mean=mean, std=std, b_mean=emean, b_std=estd)
        if not std > estd:
            res['safe'] = False                              # the decision std > 0 is within the bound
            res['margins'].append(('std', r, std, estd))
        if not std > 0 or r == max_iters:
            break
        a, c = med - lsigma * std, med + usigma * std
        ea = 2.0 * (lsigma * estd + U * lsigma * std + U * abs(a))
        ec = 2.0 * (usigma * estd + U * usigma * std + U * abs(c))
        for edge, old, err, which in ((a, lo, ea, 'lo'), (c, hi, ec, 'hi')):
            moved = edge > old - err if which == 'lo' else edge < old + err
            if moved:
                dist = float(np.abs(cur - edge).min())
                res['margins'].append((which, r, dist, err))
                if not dist > err:
                    res['safe'] = False
        nlo, nhi = max(lo, a), min(hi, c)
        inside = cur[(cur >= nlo) & (cur <= nhi)]
        if inside.size == n or inside.size == 0:
            break
        b_lo = ea if nlo != lo else b_lo
        b_hi = ec if nhi != hi else b_hi
        lo, hi, cur = nlo, nhi, inside
    res['sky'] = sky_by_rule(stat, res['med'], res['mean'], res['std'])
    return res


def check(got, st, stat, what):
    """`got`: dict of one frame's kernel results (sky med mean std lo hi n_usable n_final rounds status).  Counts,
    rounds, status and med exactly by value; lo, hi, mean, std within the statement's bounds; sky by the rule from
    the kernel's own med, mean and std."""
    assert st['safe'], (what, st['margins'])
    for k in ('n_usable', 'n_final', 'rounds', 'status'):
        assert int(got[k]) == st[k], (what, k, got[k], st[k])
    if st['status'] & EMPTY:
        for k in ('sky', 'med', 'mean', 'std'):
            assert np.isnan(got[k]), (what, k, got[k])
        return
    assert got['med'] == st['med'], (what, 'med', got['med'], st['med'])
    for k, b in (('mean', 'b_mean'), ('std', 'b_std'), ('lo', 'b_lo'), ('hi', 'b_hi')):
        if np.isinf(st[k]):
            assert got[k] == st[k], (what, k, got[k], st[k])
        else:
            assert abs(got[k] - st[k]) <= st[b], (what, k, got[k], st[k], st[b])
    exp = sky_by_rule(stat, got['med'], got['mean'], got['std'])
    assert got['sky'] == exp, (what, 'sky', got['sky'], exp)
