"""Scenes for the deblending tests (tests/test_deblend_cpu.py on the CPU harness, tests/test_gpu_deblend.py on
the device), and the numpy labelling that feeds the statement.  Not a test module itself.

Pixel values are multiples of 2^-6 and filter weights multiples of 2^-4, so the filter chain is exact in
float32 and float64 alike (deblend_statement.filtered asserts it), and the thresholds sit between two grid
values so that no pixel is within rounding of one."""
import numpy as np
from scipy import ndimage

import deblend_statement as dst

BOX = np.full((3, 3), 0.125)                    # the 3 x 3 box filter, dyadic: sums to 9/8, used as given
THR = 0.6 * 9 / 8 + 2.0 ** -9                   # 0.6 on the unit-sum box scale, off the value grid
WIDE = (np.arange(35).reshape(7, 5) % 5 + 1) / 16.0           # a 7 x 5 filter with unequal dyadic weights


def grid6(a):
    return np.round(np.asarray(a, np.float64) * 64.0) / 64.0


def gauss(shape, y, x, amp, sigma):
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    return amp * np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2.0 * sigma ** 2))


def label_np(frame, thr, mask=None, filt=None, min_area=5, conn=8):
    """(labels int32, nlabels) as spx_detect_label_* defines them, in numpy"""
    f = dst.filtered(frame, mask, filt)
    ok = np.isfinite(np.asarray(frame, np.float64))
    if mask is not None:
        ok &= ~np.asarray(mask, bool)
    lab, n = ndimage.label(ok & (f > thr), structure=dst.STRUCT[conn])
    area = np.bincount(lab.ravel(), minlength=n + 1)
    keep = area >= min_area
    keep[0] = False
    newid = np.where(keep, np.cumsum(keep), 0).astype(np.int32)
    return newid[lab], int(keep.sum())


def bboxes_np(labels, nlabels):
    """the table of spx_label_bboxes_i32: [nlabels + 1][4] = (xmin, ymin, xmax, ymax)"""
    boxes = np.tile(np.array([2 ** 31 - 1, 2 ** 31 - 1, -1, -1], np.int32), (nlabels + 1, 1))
    for l in range(1, nlabels + 1):
        ys, xs = np.nonzero(labels == l)
        if len(ys):
            boxes[l] = (xs.min(), ys.min(), xs.max(), ys.max())
    return boxes


def scene(frame, thr=THR, filt=BOX, mask=None, **kw):
    return dict(frame=frame, thr=thr, filt=filt, mask=mask, kw=kw)


def stars(shape, items, seed, noise=0.3):
    """items: (y, x, amplitude, sigma)"""
    rng = np.random.default_rng(seed)
    f = rng.normal(0.0, noise, shape) if noise else np.zeros(shape)
    for y, x, a, s in items:
        f = f + gauss(shape, y, x, a, s)
    return grid6(f)


def pair(sep, ratio=1.0, seed=1, sigma=2.5, peak=100.0, shape=(40, 56)):
    cy, cx = shape[0] / 2 - 0.5, shape[1] / 2 - 0.5
    return scene(stars(shape, [(cy, cx - sep / 2.0, peak, sigma), (cy, cx + sep / 2.0, peak * ratio, sigma)], seed))


def triple(seed=2):
    return scene(stars((44, 72), [(21, 16, 100.0, 2.5), (21, 25, 60.0, 2.5), (21, 42, 100.0, 2.5)], seed))


BUMP = (12, 16)


def weak_bump(seed=3):
    """two stars that split, and a bump of 4 at BUMP on the outskirts of the first: a branch of its own at one
    level, insignificant there"""
    return scene(stars((44, 64), [(21, 20, 100.0, 2.5), (21, 34, 100.0, 2.5), BUMP + (4.0, 1.0)], seed, noise=0.0))


def late_bloomer(seed=4):
    """a compact bright star and a broad faint one: the faint one's branch holds little flux where it appears and
    becomes significant only further down, as its component grows"""
    return scene(stars((56, 80), [(27, 24, 200.0, 1.5), (27, 37, 3.0, 5.0)], seed, noise=0.0))


def plateaus():
    """integers: two 5 x 5 plateaus of 8 joined by a bridge of 2 on a floor of 1; q ties everywhere"""
    f = np.zeros((15, 25))
    f[2:13, 2:23] = 1.0
    f[5:10, 4:9] = 8.0
    f[5:10, 16:21] = 8.0
    f[7, 9:16] = 2.0
    return scene(f, thr=0.5, filt=None)


def flat():
    f = np.zeros((12, 14))
    f[3:9, 2:11] = 4.0
    return scene(f, thr=0.5, filt=None)


def needles():
    """two 1-pixel spikes on a plateau: seeds smaller than min_area = 5"""
    f = np.zeros((13, 21))
    f[2:11, 2:19] = 10.0
    f[6, 6] = 50.0
    f[6, 14] = 50.0
    return scene(f, thr=0.5, filt=None)


def corners(seed=5):
    """pairs in the four corners, 7 x 5 filter whose halo leaves the frame"""
    ny, nx = 64, 90
    items = []
    for y in (3, ny - 4):
        for x0 in (3, nx - 16):
            items += [(y, x0, 100.0, 2.0), (y, x0 + 12, 80.0, 2.0)]
    return scene(stars((ny, nx), items, seed, noise=0.1), thr=3.0 + 2.0 ** -9, filt=WIDE)


def masked(seed=6):
    s = pair(12, 1.0, seed)
    m = np.zeros(s['frame'].shape, bool)
    m[19, 27] = True                             # between the two stars
    m[17, 22] = True                             # on the flank of the first
    s['mask'] = m
    return s


def ring(side=40, frame=(48, 52), seed=7):
    """a ring-shaped parent with two lumps on it, and other parents inside its box"""
    f = np.zeros(frame)
    y0, x0 = 3, 4
    f[y0:y0 + side, x0:x0 + side] = 6.0
    f[y0 + 2:y0 + side - 2, x0 + 2:x0 + side - 2] = 0.0
    f = f + gauss(frame, y0 + 1, x0 + 8, 60.0, 1.5) * (f > 0) + gauss(frame, y0 + 1, x0 + 30, 60.0, 1.5) * (f > 0)
    f = f + gauss(frame, y0 + 14, x0 + 13, 100.0, 2.0) + gauss(frame, y0 + 14, x0 + 25, 90.0, 2.0)
    f = f + gauss(frame, y0 + 30, x0 + 20, 50.0, 2.0)
    rng = np.random.default_rng(seed)
    return scene(grid6(f + rng.normal(0.0, 0.05, frame)), thr=1.0 + 2.0 ** -9, filt=None)


def big_ring():
    """a thin ring 260 px a side in a 300 px frame: its box is over the limit"""
    f = np.zeros((300, 300))
    f[20:280, 20:280] = 5.0
    f[21:279, 21:279] = 0.0
    f[20, 60] = 50.0
    f[20, 200] = 50.0                            # would split, were it examined
    f = f + gauss(f.shape, 150, 140, 100.0, 2.5) + gauss(f.shape, 150, 152, 100.0, 2.5)
    return scene(grid6(f), thr=1.0 + 2.0 ** -9, filt=None, min_area=1)


def blob(side, seed=8):
    """one parent of about side x side pixels with three peaks; the same shape at every side"""
    n = side + 10
    s = side / 40.0
    f = (gauss((n, n), n / 2 - 6 * s, n / 2 - 8 * s, 100.0, 3.0 * s) + gauss((n, n), n / 2 + 7 * s, n / 2 + 6 * s, 80.0, 3.0 * s)
         + gauss((n, n), n / 2 - 4 * s, n / 2 + 11 * s, 30.0, 2.0 * s))
    yy, xx = np.mgrid[0:n, 0:n]
    inside = (np.abs(yy - n / 2 + 0.5) < side / 2) & (np.abs(xx - n / 2 + 0.5) < side / 2)
    rng = np.random.default_rng(seed)
    return scene(grid6(np.where(inside, f + 1.0 + rng.uniform(0, 0.2, (n, n)), 0.0)), thr=0.5, filt=None)


def interleaved(seed=9):
    """two parents side by side, each a vertical pair: the children's first pixels interleave in raster order"""
    return scene(stars((48, 64), [(14, 16, 100.0, 2.5), (26, 16, 100.0, 2.5), (15, 44, 100.0, 2.5),
                                  (27, 44, 100.0, 2.5)], seed))


def smooth_field(seed=10, shape=(80, 96)):
    """gaussian_filter of white noise, threshold 0.3 sigma: many parents, a handful split"""
    rng = np.random.default_rng(seed)
    f = ndimage.gaussian_filter(rng.normal(size=shape), 2.5)
    f = grid6(f / f.std() * 16.0)
    return scene(f, thr=0.3 * 16.0 + 2.0 ** -9, filt=None)


def crowded(seed=11, npairs=8, shape=(200, 260)):
    """drawn close pairs on a grid of cells, positions jittered; returns the scene and the drawn centres"""
    rng = np.random.default_rng(seed)
    items = []
    cells = [(y, x) for y in range(25, shape[0] - 24, 50) for x in range(30, shape[1] - 29, 50)]
    for (y, x) in cells[:npairs]:
        y, x = y + rng.integers(-3, 4), x + rng.integers(-3, 4)
        items += [(y, x - 5, 100.0, 2.5), (y + rng.integers(-2, 3), x + 6, 70.0 + 30.0 * rng.random(), 2.5)]
    s = scene(stars(shape, items, seed))
    s['centres'] = [(int(y), int(x)) for y, x, _, _ in items]
    return s
