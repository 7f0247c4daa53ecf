"""Cosmic-ray cases for tests/test_crreject_cpu.py and tests/test_gpu_crreject.py: the smallest shapes at which the
two kernels of spx_crreject_kernels.h can go wrong.  Frame sides are 5 .. 33 and the outputs (13 x 37, 29 x 41) are no
multiples of the 32 x 8 tile.  A frame is a smooth scene sampled through its map plus Gaussian noise of sigma NOISE plus
drawn hits; every value is a float32 number, so that one float64 statement serves both frame dtypes.  The seeds are
fixed.  Not a test module.

ALL[name]() -> the dict of drizzle_cases.case plus
    rms  : per frame a scalar or a map        cr : dict(snr, scale, nlow, nhigh, sky, gain), only what differs from
    hits : [(k, j, i, amplitude)] as drawn    the defaults of crreject_statement.DEFAULTS"""
import numpy as np

from drizzle_cases import case, rot, weight

NOISE = 0.05


def scene(X, Y):
    v = 1.0 + 0.01 * X - 0.015 * Y
    for x0, y0, a in ((9.0, 5.0, 2.5), (24.0, 9.0, 1.5), (17.0, 20.0, 3.0), (31.0, 24.0, 2.0)):
        v = v + a * np.exp(-((X - x0) ** 2 + (Y - y0) ** 2) / (2 * 2.5 ** 2))
    return v


def frame(seed, ny, nx, m, noise=NOISE, flat=False):
    j, i = np.mgrid[0:ny, 0:nx].astype(np.float64)
    X, Y = m[0] * i + m[1] * j + m[2], m[3] * i + m[4] * j + m[5]
    f = np.ones((ny, nx)) if flat else scene(X, Y)
    if noise:
        f = f + noise * np.random.RandomState(seed).standard_normal((ny, nx))
    return f.astype(np.float32).astype(np.float64)


def build(seed, specs, out_shape=(13, 37), hits=(), rms=NOISE, cr=None, noise=NOISE, flat=False, **kw):
    """specs: [(ny, nx, map)]"""
    maps = [np.asarray(s[2], np.float64) for s in specs]
    frames = [frame(seed + 10 * k, s[0], s[1], maps[k], noise, flat) for k, s in enumerate(specs)]
    for k, j, i, a in hits:
        frames[k][j, i] = np.float32(frames[k][j, i] + a)
    c = case(frames, maps, out_shape=out_shape, **kw)
    c['rms'] = [rms] * len(frames) if np.isscalar(rms) else list(rms)
    c['cr'] = dict(cr or {})
    c['hits'] = list(hits)
    return c


def dithers(K, ny=12, nx=30, seed=0):
    r = np.random.RandomState(100 + seed)
    return [(ny, nx, rot(r.uniform(-2, 2), tx=r.uniform(1.5, 5.5), ty=r.uniform(0.2, 1.2), about=(nx / 2, ny / 2)))
            for _ in range(K)]


def k1():
    return build(1, dithers(1))


def k2_even():
    return build(2, dithers(2), hits=[(0, 5, 11, 1.0)])


def k3_hits():
    return build(3, dithers(3), hits=[(0, 3, 7, 1.0), (1, 8, 20, 0.8), (2, 6, 14, 1.5), (2, 6, 15, 0.9)])


def k4_nhigh():
    """two frames are hit at the same sky position: the plain median would keep half of it"""
    sp = dithers(4, seed=4)
    return build(4, sp, hits=[(0, 5, 12, 1.2), (3, 4, 21, 1.0)], cr=dict(nhigh=1))


def fallback():
    """nlow + nhigh >= m everywhere: nothing is dropped"""
    return build(5, dithers(2, seed=5), hits=[(1, 6, 9, 1.0)], cr=dict(nlow=1, nhigh=1))


def fallback_partly():
    """K = 3, nlow = nhigh = 1: trimmed where three frames overlap, not where one or two do"""
    sp = [(12, 30, rot(1.0, tx=2.5, ty=0.4)), (12, 20, rot(-1.0, tx=3.2, ty=0.7)), (8, 30, rot(0.5, tx=4.1, ty=0.3))]
    return build(6, sp, hits=[(0, 4, 8, 1.0)], cr=dict(nlow=1, nhigh=1))


def inactive_middle():
    return build(7, dithers(4, seed=7), hits=[(0, 5, 5, 1.0), (1, 5, 9, 30.0), (2, 7, 17, 1.0)], active=[1, 0, 1, 1])


def many33():
    """K = 33: the LDS column is longer than a wave's worth of slots, and K crosses a ctx word"""
    r = np.random.RandomState(33)
    sp = [(9, 11, rot(r.uniform(-3, 3), tx=r.uniform(8, 17), ty=r.uniform(1, 3), about=(5, 4))) for _ in range(33)]
    sp[:12] = [(9, 11, rot(r.uniform(-3, 3), tx=12 + r.uniform(-1, 1), ty=2 + r.uniform(-0.5, 0.5), about=(5, 4)))
               for _ in range(12)]
    return build(8, sp, hits=[(k, 4, 5, 1.0) for k in (0, 5, 32)])


def many(K):
    """K small frames over one patch of the output: K = 65 and 128 put the median's LDS column above 64 KiB (not in
    ALL: the device test of the launch's dynamic-LDS limit uses it)"""
    r = np.random.RandomState(K)
    sp = [(6, 7, rot(r.uniform(-3, 3), tx=r.uniform(12, 15), ty=r.uniform(2, 4), about=(3, 3))) for _ in range(K)]
    return build(20, sp, hits=[(0, 3, 3, 1.0)])


def geometry():
    """rotated 30 degrees, mirrored, scaled 0.5 and scaled 2"""
    sp = [(20, 25, rot(30.0, tx=8.2, ty=2.4, about=(12, 10))),
          (20, 25, rot(5.0, tx=10.4, ty=4.6, mirror=True, about=(12, 10))),
          (33, 33, rot(-4.0, scale=0.5, tx=4.3, ty=-2.1, about=(16, 16))),
          (9, 12, rot(2.0, scale=2.0, tx=9.6, ty=8.8, about=(6, 4)))]
    return build(9, sp, out_shape=(29, 41), hits=[(0, 9, 12, 1.0), (1, 10, 10, 1.0), (2, 16, 16, 1.0), (3, 4, 6, 1.0)])


def half_outside():
    """frame 0 lies half outside the output: b is undefined along a band"""
    sp = [(24, 31, rot(3.0, tx=-14.3, ty=-9.2, about=(15, 12))), (24, 31, rot(-2.0, tx=4.6, ty=2.9, about=(15, 12))),
          (24, 31, rot(1.0, tx=6.1, ty=3.3, about=(15, 12)))]
    return build(10, sp, out_shape=(29, 41), hits=[(0, 20, 25, 1.0), (0, 2, 3, 1.0), (1, 7, 7, 1.0)])


def narrow():
    """a frame narrower than the tile and one of 33 x 9: the halo crosses tile and frame edges at once"""
    sp = [(20, 5, rot(1.0, tx=15.5, ty=3.25)), (33, 9, [0, 1, 2.5, 1, 0, 1.75]), (12, 30, rot(-1.0, tx=3.3, ty=0.6)),
          (12, 30, rot(0.7, tx=2.9, ty=0.2))]
    return build(11, sp, hits=[(0, 7, 4, 1.0), (0, 8, 0, 1.0), (1, 31, 8, 1.0), (1, 32, 0, 1.0), (1, 7, 4, 1.0),
                               (1, 8, 4, 0.9)])


def positions():
    """hits at a frame corner, across a tile boundary (i = 31 | 32, j = 7 | 8), next to a masked pixel, next to a NaN
    and on a zero-weight pixel (which must not be flagged)"""
    sp = [(9, 33, rot(0.0, tx=2.25, ty=1.5)), (12, 33, rot(0.5, scale=1.25, tx=-2.25, ty=-1.25)),
          (12, 33, rot(-0.5, scale=1.25, tx=-1.4, ty=-0.9))]
    hits = [(0, 0, 0, 1.0), (0, 8, 32, 1.0), (0, 7, 31, 1.0), (0, 7, 32, 0.9), (0, 8, 31, 0.8), (1, 3, 10, 1.0),
            (1, 5, 20, 1.0), (2, 4, 15, 5.0)]
    m = np.zeros((12, 33), np.uint8)
    m[3, 11] = 1
    w = weight(12, 12, 33)
    w[4, 15] = 0.0
    c = build(12, sp, hits=hits, masks=[None, m, None], weights=[None, None, w])
    c['frames'][1][5, 21] = np.nan
    return c


def neighbour_rule():
    """a flat scene without noise and rms = 0.05, so that D ~ 0, b ~ 1 and the thresholds are 0.175 and 0.15: a
    2-pixel hit whose fainter pixel (+0.16) passes test 1 and fails test 2 -- flagged through its neighbour --, and
    an isolated pixel (+0.16) that fails test 2 only -- not flagged"""
    sp = [(12, 30, [1, 0, 3, 0, 1, 0.5]), (12, 30, [1, 0, 3.5, 0, 1, 0.25]), (12, 30, [1, 0, 2.75, 0, 1, 0.75])]
    return build(13, sp, hits=[(0, 5, 10, 1.0), (0, 5, 11, 0.16), (0, 8, 20, 0.16)], noise=0.0, flat=True)


def rms_map_nan():
    sp = dithers(3, seed=14)
    r = np.random.RandomState(14)
    maps = [(NOISE * r.uniform(0.8, 1.5, (12, 30))).astype(np.float32).astype(np.float64) for _ in range(3)]
    maps[0][3, 7] = np.nan                                      # under a hit: not testable, not flagged
    maps[1][8, 20] = -1.0
    return build(14, sp, hits=[(0, 3, 7, 1.0), (1, 8, 20, 1.0), (2, 6, 14, 1.0), (0, 9, 25, 1.0)],
                 rms=[maps[0], maps[1], NOISE])


def gain_on():
    return build(15, dithers(3, seed=15), hits=[(0, 3, 7, 1.0), (1, 8, 20, 0.4), (2, 6, 14, 2.0)],
                 cr=dict(gain=400.0, sky=0.5))


def pixfrac_half():
    return build(16, dithers(4, seed=16), hits=[(0, 3, 7, 1.0), (1, 8, 20, 0.8)], pixfrac=0.5)


def turbo():
    return build(17, dithers(3, seed=17), hits=[(0, 3, 7, 1.0), (2, 8, 20, 0.8)], kernel='turbo', pixfrac=0.8,
                 cr=dict(snr=(4.0, 2.5), scale=(1.5, 0.5)))


ALL = dict(k1=k1, k2_even=k2_even, k3_hits=k3_hits, k4_nhigh=k4_nhigh, fallback=fallback,
           fallback_partly=fallback_partly, inactive_middle=inactive_middle, many33=many33, geometry=geometry,
           half_outside=half_outside, narrow=narrow, positions=positions, neighbour_rule=neighbour_rule,
           rms_map_nan=rms_map_nan, gain_on=gain_on, pixfrac_half=pixfrac_half, turbo=turbo)
