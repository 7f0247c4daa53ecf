"""The CPU statement of deblending that tests/test_deblend_cpu.py and tests/test_gpu_deblend.py compare against
with EXACT equality: the definition of include/subpixal_hip.h (deblend block) in numpy/scipy, written from that
text and not from the kernel -- scipy.ndimage.label per level, integer sums, the flood as whole-array
synchronous sweeps.  Not a test module itself.

Two guards make exact equality a fair demand; both are test-construction errors when they fire (rebuild the
scene, take another seed), not failures of the code under test:
  * with a filter, the frame and the weights must be dyadic and small enough that every product and every
    partial sum of the filter chain is exact in the frame's dtype, so that the chain's order and fusing cannot
    matter and numpy's float64 correlation IS the device's result;
  * every x_k of the exponential levels must lie farther than 1e-5 from an integer, in case a device sqrt were
    one ulp off (the level arithmetic itself is + - * / sqrt, each correctly rounded on both sides).

What the first guard costs: because every chain is exact, NO deblending test can tell whether the device builds f
by "the same fused multiply-add chain in the frame's dtype" -- a chain in another order, or in float64, would
pass them all.  That is acceptable only because the chain is ONE device function, `det_filter_chain` in
spx_detect_kernels.h, shared by the detection and the deblending kernels, and the detection tests
(tests/test_detect_cpu.py, tests/test_gpu_detect.py) pin it with inexact weights.  Do not un-share it."""
import numpy as np
from scipy import ndimage

STRUCT = {8: np.ones((3, 3), int), 4: np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])}
SHIFTS = {4: ((0, -1), (-1, 0), (1, 0), (0, 1)),
          8: ((0, -1), (-1, 0), (1, 0), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))}
MAX_BOX_PIXELS = 65536
FLAG_DEBLENDED, FLAG_NODEBLEND = 8, 16
TWO30 = 2 ** 30
MODES = {'exponential': 0, 'linear': 1}


def _dyadic_bits(a):
    a = np.asarray(a, np.float64)
    for b in range(0, 31):
        s = a * 2.0 ** b
        if np.all(s == np.rint(s)):
            return b
    raise AssertionError("scene values are not multiples of 2^-30: the filter chain would round")


def filtered(frame, mask=None, filt=None):
    """f of the definition, float64 (exactly what the device computes in the frame's dtype: see the guard)"""
    frame = np.asarray(frame)
    v = frame.astype(np.float64)
    ok = np.isfinite(v)
    if mask is not None:
        ok &= ~np.asarray(mask, bool)
    vp = np.where(ok, v, 0.0)
    if filt is None:
        return vp
    k = np.asarray(filt, np.float64)
    assert k.ndim == 2 and k.shape[0] % 2 == 1 and k.shape[1] % 2 == 1
    bits = _dyadic_bits(vp) + _dyadic_bits(k)
    mag = ndimage.correlate(np.abs(vp), np.abs(k), mode='constant', cval=0.0)
    digits = 53 if frame.dtype == np.float64 else 24
    assert mag.max() * 2.0 ** bits < 2.0 ** digits, "the filter chain would round in the frame's dtype"
    return ndimage.correlate(vp, k, mode='constant', cval=0.0)


def levels(lo, hi, n, mode, margin=None):
    """TQ_0..TQ_n as Python integers.  margin: a list that receives every x_k's distance from the nearest integer
    (exponential levels below 2^30 only: the values the 1e-5 guard looks at)"""
    assert mode in (0, 1) and n + 1 in (2, 4, 8, 16, 32, 64)
    lo, hi = np.float64(lo), np.float64(hi)
    with np.errstate(all='ignore'):
        rho = hi / lo if (mode == 0 and lo > 0.0) else np.float64(np.nan)
    if np.isfinite(rho):
        g = rho
        for _ in range(int(np.log2(n + 1))):
            g = np.sqrt(g)
        tq, p = [0], np.float64(1.0)
        for k in range(1, n + 1):
            p = p * g
            with np.errstate(all='ignore'):
                x = ((p - np.float64(1.0)) / (rho - np.float64(1.0))) * np.float64(TWO30)
            if not x < TWO30:
                tq.append(TWO30)
                continue
            if margin is not None:
                margin.append(float(abs(x - np.rint(x))))
            assert abs(x - np.rint(x)) > 1e-5, "level %d: x_k = %r is within 1e-5 of an integer" % (k, x)
            tq.append(int(min(np.float64(TWO30), np.ceil(x))))
        return tq
    return [k * TWO30 // (n + 1) for k in range(n + 1)]


def _objects(q, P, tq, conn, contrast, min_area, trace=None):
    """the seeds of one parent (boolean masks over the box), in no particular order.  trace: a list that receives
    one record per child examined, dict(level = the child's own level, mask, npix, flux, share = flux / F(P),
    has_objs, significant), for tests that want to see WHY a scene splits"""
    n = len(tq) - 1
    FP = int(q[P].sum())
    prev_lab, prev_objs = None, None
    for k in range(n, -1, -1):
        lab, nc = ndimage.label(P & (q >= tq[k]), structure=STRUCT[conn])
        objs = {}
        for c in range(1, nc + 1):
            C = lab == c
            children = [] if prev_lab is None else [d for d in np.unique(prev_lab[C]) if d]
            sig = []
            for d in children:
                D = prev_lab == d
                isig = bool(prev_objs[d]) or (float(int(q[D].sum())) >= contrast * float(FP) and int(D.sum()) >= min_area)
                if isig:
                    sig.append(d)
                if trace is not None:
                    trace.append(dict(level=k + 1, mask=D, npix=int(D.sum()), flux=int(q[D].sum()),
                                      share=int(q[D].sum()) / FP, has_objs=bool(prev_objs[d]), significant=isig))
            if len(sig) >= 2:
                objs[c] = []
                for d in sig:
                    objs[c] += prev_objs[d] if prev_objs[d] else [prev_lab == d]
            else:
                ne = [prev_objs[d] for d in children if prev_objs[d]]
                assert len(ne) <= 1
                objs[c] = ne[0] if ne else []
        prev_lab, prev_objs = lab, objs
    seeds = []
    for c in sorted(prev_objs):
        seeds += prev_objs[c]
    return seeds


def _flood(q, P, tq, conn, seeds):
    seeds = sorted(seeds, key=lambda m: np.flatnonzero(m.ravel())[0])
    o = np.zeros(P.shape, np.int64)
    for i, m in enumerate(seeds):
        assert not o[m].any()
        o[m] = i + 1
    h, w = P.shape
    for k in range(len(tq) - 1, -1, -1):
        while True:
            po = np.pad(o, 1)
            pq = np.pad(q, 1, constant_values=-1)
            bq = np.full(P.shape, -1, np.int64)
            bo = np.zeros(P.shape, np.int64)
            for dy, dx in SHIFTS[conn]:
                no = po[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
                nq = pq[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
                better = (no > 0) & ((nq > bq) | ((nq == bq) & (no < bo)))
                bq = np.where(better, nq, bq)
                bo = np.where(better, no, bo)
            take = P & (o == 0) & (q >= tq[k]) & (bo > 0)
            if not take.any():
                break
            o[take] = bo[take]
    return o


def statement(frame, labels, nlabels, mask=None, filt=None, levels_n=31, contrast=0.005, mode='exponential',
              min_area=5, conn=8, trace=None):
    """dict(labels int32 [ny, nx], n, parent int32 [n], dflags int32 [n], split = the input labels that were split).
    trace: a dict that receives, per examined parent label, (y0, x0 of its box, the records of _objects)"""
    mode = MODES.get(mode, mode)
    f = filtered(frame, mask, filt)
    labels = np.asarray(labels)
    segs = []                                    # (first pixel, ys, xs, parent, flag)
    split = []
    for l in range(1, nlabels + 1):
        ys, xs = np.nonzero(labels == l)
        if not len(ys):
            continue
        y0, y1, x0, x1 = ys.min(), ys.max(), xs.min(), xs.max()
        P = labels[y0:y1 + 1, x0:x1 + 1] == l
        fb = f[y0:y1 + 1, x0:x1 + 1]
        o = None
        flag = 0
        if P.size > MAX_BOX_PIXELS:
            flag = FLAG_NODEBLEND
        else:
            lo, hi = fb[P].min(), fb[P].max()
            if hi > lo:
                q = np.minimum(np.float64(TWO30), np.floor(((fb - lo) / (hi - lo)) * np.float64(TWO30)))
                q = np.where(P, q, -1).astype(np.int64)
                tq = levels(lo, hi, levels_n, mode)
                rec = None if trace is None else []
                seeds = _objects(q, P, tq, conn, contrast, min_area, rec)
                if trace is not None:
                    trace[l] = (y0, x0, rec)
                if seeds:
                    o = _flood(q, P, tq, conn, seeds)
        if o is None:
            segs.append((ys[0] * labels.shape[1] + xs[0], ys, xs, l, flag))
            continue
        split.append(l)
        for i in np.unique(o[P]):                # 0: pixels no seed reached (a parent that is not connected)
            cy, cx = np.nonzero(P & (o == i))
            segs.append(((cy[0] + y0) * labels.shape[1] + cx[0] + x0, cy + y0, cx + x0, l, FLAG_DEBLENDED))
    segs.sort(key=lambda s: s[0])
    out = np.zeros(labels.shape, np.int32)
    for i, (_, ys, xs, _, _) in enumerate(segs):
        out[ys, xs] = i + 1
    return dict(labels=out, n=len(segs), parent=np.array([s[3] for s in segs], np.int32).reshape(-1),
                dflags=np.array([s[4] for s in segs], np.int32).reshape(-1), split=split)


def check(got_labels, got_n, got_parent, got_dflags, st, what=''):
    """exact equality of all three arrays; there is no tolerance anywhere"""
    assert got_n == st['n'], "%s: %d segments, the statement has %d" % (what, got_n, st['n'])
    nd = int((np.asarray(got_labels) != st['labels']).sum())
    assert nd == 0, "%s: label image differs from the statement's at %d pixels" % (what, nd)
    assert np.array_equal(np.asarray(got_parent)[:got_n], st['parent']), what
    assert np.array_equal(np.asarray(got_dflags)[:got_n], st['dflags']), what
