"""Drizzle cases for tests/test_drizzle_cpu.py and tests/test_gpu_drizzle.py: the smallest shapes at which the kernel
can go wrong.  Frames are 5 x 7 .. 24 x 31 and the outputs (37 x 53 and the like) are no multiples of the 32 x 8 output
tile.  Every pixel value and weight is a float32 number, so that one float64 statement serves both frame dtypes.
Not a test module.  ALL[name]() -> dict(frames, maps, out_shape, weights, masks, active, pixfrac, kernel, fill)."""
import numpy as np


def frame(seed, ny, nx):
    r = np.random.RandomState(seed)
    return (r.uniform(-1.0, 3.0, (ny, nx)).astype(np.float32)).astype(np.float64)


def weight(seed, ny, nx):
    r = np.random.RandomState(1000 + seed)
    return (r.uniform(0.25, 2.0, (ny, nx)).astype(np.float32)).astype(np.float64)


def rot(deg, scale=1.0, tx=0.0, ty=0.0, mirror=False, about=(0.0, 0.0)):
    """rotation by `deg` and `scale` about the input point `about`, which lands on (tx, ty) + about"""
    c, s = np.cos(np.deg2rad(deg)) * scale, np.sin(np.deg2rad(deg)) * scale
    a = np.array([[c, -s], [s, c]])
    if mirror:
        a = a @ np.array([[-1.0, 0.0], [0.0, 1.0]])
    ab = np.asarray(about, np.float64)
    t = ab + (tx, ty) - a @ ab
    return np.array([a[0, 0], a[0, 1], t[0], a[1, 0], a[1, 1], t[1]])


def case(frames, maps, out_shape=(37, 53), weights=None, masks=None, active=None, pixfrac=1.0, kernel='square',
         fill=0.0):
    return dict(frames=frames, maps=[np.asarray(m, np.float64) for m in maps], out_shape=out_shape, weights=weights,
                masks=masks, active=active, pixfrac=pixfrac, kernel=kernel, fill=fill)


def identity():
    return case([frame(1, 24, 31)], [[1, 0, 0, 0, 1, 0]], weights=[weight(1, 24, 31)])


def identity_full():
    """the frame is the output grid: every output pixel is one input pixel"""
    return case([frame(2, 19, 23)], [[1, 0, 0, 0, 1, 0]], out_shape=(19, 23), weights=[weight(2, 19, 23)])


def integer_shifts():
    return case([frame(3, 12, 17), frame(4, 9, 14)], [[1, 0, 5, 0, 1, 3], [1, 0, 24, 0, 1, 16]],
                weights=[weight(3, 12, 17), weight(4, 9, 14)])


def twice():
    return case([frame(5, 11, 13)], [[2, 0, 2.5, 0, 2, 3.5]])


def twice_half_drop():
    return case([frame(5, 11, 13)], [[2, 0, 2.5, 0, 2, 3.5]], pixfrac=0.5)


def rot_tiny():
    return case([frame(6, 24, 31)], [rot(0.002, tx=3.3, ty=4.7, about=(15, 12))], weights=[weight(6, 24, 31)])


def rot30():
    return case([frame(7, 20, 25)], [rot(30.0, tx=12.2, ty=6.4, about=(12, 10))], weights=[weight(7, 20, 25)])


def rot90():
    return case([frame(8, 24, 31)], [[0, -1, 30.25, 1, 0, 2.5]], fill=-7.0)


def shrink():
    return case([frame(9, 24, 31)], [rot(11.0, scale=0.5, tx=9.1, ty=8.3, about=(15, 12))], weights=[weight(9, 24, 31)])


def grow():
    return case([frame(10, 10, 12)], [rot(-23.0, scale=2.0, tx=12.7, ty=9.9, about=(6, 5))])


def mirrored():
    return case([frame(11, 20, 25)], [rot(17.0, scale=1.1, tx=10.4, ty=7.6, mirror=True, about=(12, 10))],
                weights=[weight(11, 20, 25)])


def half_outside():
    return case([frame(12, 24, 31), frame(13, 24, 31)],
                [rot(5.0, tx=-16.3, ty=-11.2, about=(15, 12)), rot(-5.0, tx=37.6, ty=24.9, about=(15, 12))])


def misses():
    return case([frame(14, 8, 9), frame(15, 8, 9)], [[1, 0, 200.5, 0, 1, 3.25], [1, 0, 10.5, 0, 1, 3.25]])


def small_frame():
    """5 x 7: smaller than one 32 x 8 tile, and astride the corner of four of them"""
    return case([frame(16, 5, 7)], [rot(3.0, tx=28.4, ty=5.3, about=(3, 2))])


def pixfrac_tenth():
    return case([frame(17, 20, 25)], [rot(7.0, scale=1.5, tx=6.2, ty=4.9, about=(12, 10))], pixfrac=0.1, fill=-1.0)


def bad_weights():
    w = weight(18, 20, 25)
    w[::3, ::4] = 0.0
    w[1::5, 2::3] = np.nan
    w[2::4, 1::5] = -1.0
    w[7, 7] = np.inf
    return case([frame(18, 20, 25)], [rot(2.0, tx=5.5, ty=6.5, about=(12, 10))], weights=[w])


def nan_data():
    d = frame(19, 20, 25)
    d[::4, ::3] = np.nan
    d[5, 5] = np.inf
    d[6, 6] = -np.inf
    return case([d], [rot(-2.0, tx=5.5, ty=6.5, about=(12, 10))], weights=[weight(19, 20, 25)])


def masked():
    m = np.zeros((20, 25), np.uint8)
    m[3:9, 4:12] = 1
    m[15, :] = 200
    return case([frame(20, 20, 25), frame(21, 20, 25)],
                [rot(1.0, tx=5.5, ty=6.5, about=(12, 10)), rot(-1.0, tx=8.25, ty=7.75, about=(12, 10))],
                weights=[weight(20, 20, 25), None], masks=[m, None])


def many_frames():
    """K = 33: two ctx planes"""
    r = np.random.RandomState(5)
    maps = [rot(r.uniform(-20, 20), tx=r.uniform(0, 44), ty=r.uniform(0, 28)) for _ in range(33)]
    return case([frame(30 + k, 8, 8) for k in range(33)], maps, weights=[weight(30 + k, 8, 8) for k in range(33)])


def mixed_shapes():
    return case([frame(22, 24, 31), frame(23, 5, 7), frame(24, 13, 9)],
                [rot(4.0, tx=4.4, ty=3.3, about=(15, 12)), rot(-30.0, tx=30.5, ty=20.5, about=(3, 2)),
                 rot(60.0, scale=1.3, tx=20.1, ty=10.2, about=(4, 6))],
                weights=[weight(22, 24, 31), None, weight(24, 13, 9)])


def inactive():
    c = mixed_shapes()
    c['active'] = [1, 0, 1]
    return c


def turbo():
    return case([frame(25, 20, 25), frame(26, 20, 25)],
                [rot(30.0, scale=0.8, tx=12.2, ty=6.4, about=(12, 10)), rot(0.0, tx=7.5, ty=9.25)],
                weights=[weight(25, 20, 25), weight(26, 20, 25)], kernel='turbo', pixfrac=0.8)


def point():
    return case([frame(27, 20, 25), frame(28, 20, 25)],
                [rot(30.0, scale=1.4, tx=12.2, ty=6.4, about=(12, 10)), rot(0.0, tx=7.5, ty=9.25)],
                weights=[weight(27, 20, 25), None], kernel='point', fill=9.0)


ALL = dict(identity=identity, identity_full=identity_full, integer_shifts=integer_shifts, twice=twice,
           twice_half_drop=twice_half_drop, rot_tiny=rot_tiny, rot30=rot30, rot90=rot90, shrink=shrink, grow=grow,
           mirrored=mirrored, half_outside=half_outside, misses=misses, small_frame=small_frame,
           pixfrac_tenth=pixfrac_tenth, bad_weights=bad_weights, nan_data=nan_data, masked=masked,
           many_frames=many_frames, mixed_shapes=mixed_shapes, inactive=inactive, turbo=turbo, point=point)
# the three the device is compared with the CPU harness on, bit for bit
BITWISE = ('rot30', 'many_frames', 'mirrored')
