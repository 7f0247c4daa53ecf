"""Scenes for the error measurements (tests/test_errors_cpu.py, tests/test_gpu_errors.py): small frames with
hand-placed segments.  A scene is dict(frame float64, labels int32, n, rms, bkg, gain, mask); frame, rms and bkg
are cast to the dtype under test by the caller, so both sides see the same numbers.  Not a test module itself."""
import numpy as np
from scipy import ndimage


def gauss(shape, y, x, amp, sigma):
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    return amp * np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2.0 * sigma ** 2))


def label(on):
    lab, n = ndimage.label(on, structure=np.ones((3, 3), int))
    return lab.astype(np.int32), int(n)


def scene(frame, labels, n, rms, bkg=0.0, gain=None, mask=None):
    return dict(frame=np.asarray(frame, np.float64), labels=np.ascontiguousarray(labels, np.int32), n=int(n), rms=rms,
                bkg=bkg, gain=gain, mask=mask)


def noisy(shape, seed, sigma=0.05):
    return np.random.default_rng(seed).normal(0.0, sigma, shape)


def one_pixel():
    f = noisy((8, 9), 1)
    f[3, 4] = 5.0
    lab = np.zeros(f.shape, np.int32)
    lab[3, 4] = 1
    return scene(f, lab, 1, 0.05)


def big_boxes():
    """a 26 x 27 box (702 px, more than one pass of 256 threads) and a 47 x 61 one (2867 px), rms a map"""
    f = noisy((96, 96), 2) + gauss((96, 96), 20, 22, 30.0, 4.0) + gauss((96, 96), 62, 50, 50.0, 9.0)
    f[55:70, 30:75] += 3.0
    lab, n = label(f > 1.0)
    assert n == 2
    rms = 0.05 + 0.01 * np.sin(np.arange(96) / 7.0)[None, :] * np.ones((96, 1))
    return scene(f, lab, n, rms, bkg=0.01)


def ring():
    """a square ring (label 1) with two other labels inside its box"""
    f = noisy((40, 44), 3)
    on = np.zeros(f.shape, bool)
    on[4:36, 5:39] = True
    on[6:34, 7:37] = False
    f[on] += 4.0 + 0.1 * np.arange(on.sum())
    f += gauss(f.shape, 14, 15, 20.0, 1.5) + gauss(f.shape, 25, 28, 12.0, 2.0)
    lab, n = label(f > 1.0)
    assert n == 3
    return scene(f, lab, n, 0.05, gain=4.0)


def bad_pixels():
    """a masked and a NaN pixel inside a segment, an Inf pixel inside its box but outside the segment"""
    f = noisy((30, 33), 4) + gauss((30, 33), 14, 16, 40.0, 3.0)
    lab, n = label(f > 1.0)
    assert n == 1
    mask = np.zeros(f.shape, bool)
    mask[13, 15] = True
    f[16, 18] = np.nan
    ys, xs = np.nonzero(lab)
    corner = (ys.min(), xs.min())
    assert lab[corner] == 0
    f[corner] = np.inf
    return scene(f, lab, n, 0.05, mask=mask, gain=2.0)


def bad_rms():
    """three segments, each with one rms pixel that is 0, negative or NaN; a fourth with a clean map"""
    shape = (40, 60)
    f = noisy(shape, 5)
    cents = [(10, 10), (10, 40), (28, 12), (28, 44)]
    for y, x in cents:
        f += gauss(shape, y, x, 25.0, 2.5)
    lab, n = label(f > 1.0)
    assert n == 4
    rms = np.full(shape, 0.05) + 0.001 * (np.arange(shape[1]) % 5)[None, :]
    rms[10, 10], rms[10, 41], rms[29, 12] = 0.0, -0.05, np.nan
    return scene(f, lab, n, rms, gain=3.0)


def negative_w(gain=None):
    """a background above the segment's outskirts: negative w inside the segment (no shot noise there)"""
    f = noisy((32, 32), 6) + gauss((32, 32), 15, 16, 30.0, 3.5)
    lab, n = label(f > 0.5)
    assert n == 1
    s = scene(f, lab, n, 0.05, bkg=2.0, gain=gain)
    assert ((f - 2.0)[lab == 1] < 0).sum() > 10 and (f - 2.0)[lab == 1].sum() > 0
    return s


def no_flux():
    """one segment (the first) whose every pixel lies below its background, one with flux > 0"""
    f = noisy((24, 40), 7) + gauss((24, 40), 11, 9, 30.0, 2.0) + gauss((24, 40), 12, 28, 3.0, 2.0)
    lab, n = label(f > 1.0)
    assert n == 2
    bkg = np.zeros(f.shape)
    bkg[:, :20] = 50.0
    assert (f - bkg)[lab == 1].max() < 0
    return scene(f, lab, n, 0.05, bkg=bkg, gain=1.5)


def border():
    """segments on the four borders and in a corner"""
    shape = (36, 41)
    f = noisy(shape, 8)
    for y, x in ((0, 0), (0, 20), (17, 40), (35, 20), (17, 0), (18, 20)):
        f += gauss(shape, y, x, 20.0, 2.0)
    lab, n = label(f > 1.0)
    assert n == 6
    return scene(f, lab, n, 0.04 + 0.0 * f, gain=2.0)


def plateau():
    """a flat-topped segment: the peak is tied over 12 pixels; and a wholly flat one (every pixel >= half
    maximum: FLAG_HALFMAX)"""
    f = np.zeros((24, 40))
    f[5:17, 4:18] = 2.0
    f[8:11, 9:13] = 8.0
    f[6:12, 25:33] = 3.0
    lab, n = label(f > 1.0)
    assert n == 2
    return scene(f, lab, n, 0.125, gain=2.0)


def empty():
    f = noisy((12, 13), 9)
    return scene(f, np.zeros(f.shape, np.int32), 0, 0.05)


def single_pixel_frame():
    return scene(np.array([[3.0]]), np.ones((1, 1), np.int32), 1, 0.5, gain=2.0)


def field(ny=256, nx=256, seed=21):
    """smoothed noise over a slowly varying sky, an rms map, a few masked / NaN pixels and bad rms pixels"""
    rng = np.random.default_rng(seed)
    g = ndimage.gaussian_filter(rng.standard_normal((ny, nx)), 2.5, mode='wrap')
    g = g / g.std()
    lab, n = label(g > 1.1)
    bkg = -4.0 + 0.5 * np.sin(np.arange(nx) / 40.0)[None, :] * np.ones((ny, 1))
    rms = 0.05 * (1.0 + 0.3 * np.cos(np.arange(ny) / 30.0))[:, None] * np.ones((1, nx))
    rms[rng.random((ny, nx)) < 1e-3] = np.nan
    rms[rng.random((ny, nx)) < 1e-3] = -1.0
    mask = rng.random((ny, nx)) < 2e-3
    f = (g - 0.8) + bkg                         # w = g - 0.8: most segments reach below half their maximum
    f[rng.random((ny, nx)) < 1e-3] = np.nan
    return scene(f, lab, n, rms, bkg=bkg, gain=5.0, mask=mask)


ALL = dict(one_pixel=one_pixel, big_boxes=big_boxes, ring=ring, bad_pixels=bad_pixels, bad_rms=bad_rms,
           negative_w_gain_off=negative_w, negative_w_gain_on=lambda: negative_w(2.0), no_flux=no_flux, border=border,
           plateau=plateau, empty=empty, single_pixel_frame=single_pixel_frame)
