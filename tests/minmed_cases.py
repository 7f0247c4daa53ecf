"""Cases for tests/test_minmed_cpu.py and tests/test_gpu_minmed.py, on the conventions of drizzle_cases.py and
crreject_cases.py (a case is crreject_cases.build's dict; every value is a float32 number).  Outputs are 45 x 70: the
32 x 8 tile is crossed in both directions and the last tile is partial.  Not a test module.

COMBINE[name]() -> a case for step 2', plus `mm` = dict(nsigma, grow) where that differs from the defaults and, where
    the rows' combine_rms differ from rms, `combine_rms`.
GROW[name]() -> a case for step 7, plus `grow` = [(g, c, ctedir)], the settings to run it with.
The `planted` cases are flat, noise-free scenes on integer maps, so that a single-frame value is a frame's pixel and
every decision can be placed by hand: a hit of +1.0 is a seed, one of +0.34 (t = 0.17 between 3 and 4 sigma of
rms = 0.05 at K = 2) passes the second test only."""
import numpy as np

import crreject_cases as cc
from drizzle_cases import rot, weight

OUT = (45, 70)
IDENT = [1, 0, 0, 0, 1, 0]
# seeds at output pixels x = 31 | 32 and y = 7 | 8, on the border and in a corner
SEEDS = [(7, 31), (8, 32), (0, 20), (44, 69), (20, 0), (30, 50)]
# second-test-only pixels at Chebyshev distance 1, 8 and 9 of a seed, across tile borders and at the grid's edge
FAINT = [(7, 32), (8, 31), (6, 30), (16, 40), (15, 23), (30, 58), (30, 59), (22, 42), (21, 41), (1, 21), (43, 68),
         (28, 0), (29, 1), (40, 10)]


def dithers(K, ny=40, nx=64, seed=0):
    r = np.random.RandomState(200 + seed)
    return [(ny, nx, rot(r.uniform(-2, 2), tx=r.uniform(1.5, 5.5), ty=r.uniform(0.5, 4.0), about=(nx / 2, ny / 2)))
            for _ in range(K)]


def hits_of(seed, K, n, ny=40, nx=64, amp=(0.6, 1.5)):
    r = np.random.RandomState(300 + seed)
    return [(int(r.randint(K)), int(r.randint(ny)), int(r.randint(nx)), float(np.float32(r.uniform(*amp))))
            for _ in range(n)]


def build(seed, specs, mm=None, grow=None, combine_rms=None, **kw):
    kw.setdefault('out_shape', OUT)
    c = cc.build(seed, specs, **kw)
    c['mm'] = dict(mm or {})
    if grow is not None:
        c['grow'] = list(grow)
    if combine_rms is not None:
        c['combine_rms'] = list(combine_rms)
    return c


def planted(grow):
    def make():
        sp = [(45, 70, IDENT), (45, 70, IDENT)]
        hits = [(0, y, x, 1.0) for y, x in SEEDS] + [(0, y, x, 0.34) for y, x in FAINT]
        return build(40, sp, mm=dict(grow=grow), hits=hits, noise=0.0, flat=True)
    return make


def k2():
    return build(41, dithers(2, seed=1), hits=hits_of(1, 2, 12))


def k3_gain():
    return build(42, dithers(3, seed=2), hits=hits_of(2, 3, 14), cr=dict(gain=400.0, sky=0.5),
                 mm=dict(grow=2, nsigma=(1.0, 0.5)))


def k5_trim():
    """nlow and nhigh non-zero; where fewer than three frames overlap nothing is trimmed"""
    return build(43, dithers(5, seed=3), hits=hits_of(3, 5, 16), cr=dict(nlow=1, nhigh=2), mm=dict(nsigma=(1.5, 1.0)))


def k3_inactive_weight():
    """row 1 is inactive (its hit of 30 must not be seen) and row 2 has a weight map with zeros"""
    sp = dithers(4, seed=4)
    w = weight(44, 40, 64)
    w[10:14, 20:30] = 0.0
    return build(44, sp, hits=hits_of(4, 4, 12) + [(1, 12, 12, 30.0)], active=[1, 0, 1, 1],
                 weights=[None, None, w, None], combine_rms=[0.05, 0.5, 0.06, 0.04], mm=dict(nsigma=(1.0, 0.6)))


def small_frames():
    """frames much smaller than the output: pixels with m = 0, 1, 2 and 3"""
    sp = [(20, 30, rot(1.0, tx=5.5, ty=3.25)), (25, 28, rot(-1.5, tx=18.2, ty=9.6)), (18, 40, rot(0.5, tx=22.4, ty=20.1))]
    return build(45, sp, hits=hits_of(5, 3, 9, ny=18, nx=28), mm=dict(nsigma=(2.0, 1.0)))


def ties():
    """four equal frames (flat, no noise), rows 0 and 3 hit at the same pixels: md = 1.5 there and the minimum 1 is
    supplied by rows 1 and 2, whose combine_rms differ so much that only kmin = 1 makes the pixel a seed"""
    sp = [(45, 70, IDENT)] * 4
    hits = [(k, y, x, 1.0) for y, x in SEEDS for k in (0, 3)]
    return build(46, sp, hits=hits, noise=0.0, flat=True, combine_rms=[10.0, 0.01, 10.0, 10.0])


def many65():
    """K = 65 small frames over one patch: the LDS column is 65 KiB"""
    r = np.random.RandomState(65)
    sp = [(6, 7, rot(r.uniform(-3, 3), tx=r.uniform(12, 15), ty=r.uniform(2, 4), about=(3, 3))) for _ in range(65)]
    return build(47, sp, out_shape=(13, 37), hits=[(0, 3, 3, 1.0), (7, 2, 4, 1.0)], mm=dict(nsigma=(2.0, 1.0)))


COMBINE = dict(planted_grow0=planted(0), planted_grow1=planted(1), planted_grow8=planted(8), k2=k2, k3_gain=k3_gain,
               k5_trim=k5_trim, k3_inactive_weight=k3_inactive_weight, small_frames=small_frames, ties=ties,
               many65=many65)

# step 7 ----------------------------------------------------------------------------------------------------------
SETTINGS = [(3, 0, 0), (9, 0, 0), (1, 5, 1), (3, 5, -1), (1, 64, 1), (9, 64, -1), (3, 64, 0)]


def grow_planted():
    """three flat frames; frame 0 is shifted by -3 px, so its columns 0 .. 2 have no b.  Seeds of frame 0 at
    x = 31 | 32, y = 7 | 8, on three borders, next to the columns without b and next to a masked pixel"""
    sp = [(40, 64, [1, 0, -3, 0, 1, 2]), (45, 70, IDENT), (45, 70, IDENT)]
    hits = [(0, 7, 31, 1.0), (0, 8, 32, 1.0), (0, 0, 20, 1.0), (0, 39, 63, 1.0), (0, 20, 4, 1.0), (0, 25, 50, 1.0),
            (0, 39, 10, 1.0), (1, 7, 32, 1.0), (2, 30, 0, 1.0)]
    m = np.zeros((40, 64), np.uint8)
    m[25, 51] = m[24, 50] = m[27, 50] = 1
    return build(50, sp, hits=hits, noise=0.0, flat=True, masks=[m, None, None], grow=SETTINGS)


def grow_dithered():
    """noise, rotation, a weight map with zeros and an rms map with a NaN next to hits"""
    sp = dithers(3, seed=6)
    w = weight(51, 40, 64)
    w[15:18, 30:34] = 0.0
    rm = np.full((40, 64), cc.NOISE, np.float32).astype(np.float64)
    rm[9, 40] = np.nan
    hits = [(0, 16, 29, 1.5), (0, 16, 34, 1.5), (1, 9, 41, 1.5), (1, 8, 31, 1.2), (2, 7, 32, 1.2), (2, 39, 0, 1.5)]
    return build(51, sp, hits=hits + hits_of(6, 3, 8), weights=[w, None, None], rms=[cc.NOISE, rm, cc.NOISE],
                 grow=[(3, 5, 1), (9, 64, -1)])


GROW = dict(grow_planted=grow_planted, grow_dithered=grow_dithered)


# the reason for the feature -----------------------------------------------------------------------------------
def visit2():
    """K = 2 on a 96 x 96 output, hits drawn into frame 0 only.  A hit is a Gaussian profile (sigma 2 px, peak 30 .. 60
    times the noise) cut off at 7 px, as a cosmic ray with wings; `core` marks its pixels above half the peak, the
    "drawn hit pixels" the tests count.  No two hits within 16 px of each other."""
    sp = [(90, 90, rot(0.3, tx=2.4, ty=3.3, about=(45, 45))), (90, 90, rot(-0.2, tx=3.7, ty=2.6, about=(45, 45)))]
    c = build(96, sp, out_shape=(96, 96))
    r = np.random.RandomState(96)
    centres = []
    while len(centres) < 12:
        j, i = r.uniform(10, 80), r.uniform(10, 80)
        if all(max(abs(j - q[0]), abs(i - q[1])) > 16 for q in centres):
            centres.append((j, i, r.uniform(1.5, 3.0)))
    jj, ii = np.mgrid[0:90, 0:90].astype(np.float64)
    core = np.zeros((90, 90), bool)
    f = c['frames'][0]
    for j, i, a in centres:
        r2 = (jj - j) ** 2 + (ii - i) ** 2
        prof = np.where(r2 <= 49.0, np.exp(-r2 / 8.0), 0.0)
        f += a * prof
        core |= prof >= 0.5
    c['frames'][0] = f.astype(np.float32).astype(np.float64)
    c['core'] = core
    return c
