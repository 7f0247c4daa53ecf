"""Cases for the drizzle through polynomial maps (tests/test_drizzle_poly_cpu.py, tests/test_gpu_drizzle_poly.py): frames
of about 40 x 48 with differing shapes onto outputs such as 37 x 70 -- no multiple of the 32 x 8 tile and more than
two tiles per axis, the smallest size at which the tile skip, partial tiles and the candidate window can go wrong.
Every pixel value and weight is a float32 number, so that one float64 statement serves both frame dtypes.
Not a test module.  ALL[name]() -> dict(frames, maps, out_shape, weights, masks, active, pixfrac, kernel, fill); a map
is a ``[6]`` array or a ``resample.PolyMap``."""
import numpy as np

from drizzle_cases import frame, rot, weight

OUT = (37, 70)


def _slot(i, j):
    return (i + j) * (i + j + 1) // 2 + j


def distorted(ny, nx, deg=20.0, scale=0.95, tx=30.0, ty=18.0, k=5.1e-5, q=(6e-4, -4e-4), mirror=False, degree=3):
    """rotation o (scale (1 + k r^2) (u, v) + (q0, q1) u v) about the frame's centre, which lands on (tx, ty): a radial
    cubic (area factor 1 .. 1 + 4 k r^2) and degree-2 cross terms, so the drops are no parallelograms"""
    from subpixal_amd.resample import PolyMap
    f = np.zeros((2, 21))
    f[0, _slot(1, 0)] = -scale if mirror else scale
    f[1, _slot(0, 1)] = scale
    if degree >= 3:
        sg = -1.0 if mirror else 1.0
        f[0, _slot(3, 0)] = f[0, _slot(1, 2)] = sg * scale * k
        f[1, _slot(2, 1)] = f[1, _slot(0, 3)] = scale * k
    if degree >= 2:
        f[0, _slot(1, 1)], f[1, _slot(1, 1)] = q
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    coef = np.stack([c * f[0] - s * f[1], s * f[0] + c * f[1]])
    coef[0, 0], coef[1, 0] = tx, ty
    return PolyMap(coef, degree, (0.5 * (nx - 1), 0.5 * (ny - 1)))


def case(frames, maps, out_shape=OUT, weights=None, masks=None, active=None, pixfrac=1.0, kernel='square', fill=0.0):
    return dict(frames=frames, maps=list(maps), out_shape=out_shape, weights=weights, masks=masks, active=active,
                pixfrac=pixfrac, kernel=kernel, fill=fill)


AFFINE1 = rot(17.0, scale=0.9, tx=11.3, ty=-2.6, about=(23.5, 19.5))


def degree1():
    """a degree-1 PolyMap of a rotated and scaled affine (also run through the affine entries: affine_twin)"""
    from subpixal_amd.resample import PolyMap
    return case([frame(101, 40, 48)], [PolyMap.from_affine(AFFINE1, (23.5, 19.5))], weights=[weight(101, 40, 48)])


def affine_twin():
    """degree1's inputs with the map as a [6] array, for the affine kernel"""
    return dict(degree1(), maps=[AFFINE1])


def radial3(**over):
    """degree 3, +-10 % area change, cross terms; weights with a zero, a negative and a NaN, a NaN pixel, a mask"""
    d, w = frame(102, 40, 48), weight(102, 40, 48)
    w[3, 5], w[7, 9], w[11, 13] = 0.0, -1.0, np.nan
    d[20, 20] = np.nan
    m = np.zeros((40, 48), np.uint8)
    m[28:33, 6:15] = 1
    c = case([d], [distorted(40, 48)], weights=[w], masks=[m])
    c.update(over)
    return c


def radial3_p06():
    return radial3(pixfrac=0.6)


def radial3_turbo():
    return radial3(kernel='turbo', pixfrac=0.8)


def radial3_point():
    return radial3(kernel='point', fill=9.0)


def degree5():
    """all 21 slots of both axes non-zero, magnitudes falling with the degree"""
    from subpixal_amd.resample import PolyMap
    r = np.random.RandomState(7)
    coef = distorted(41, 45, deg=-12.0, scale=1.05, tx=36.0, ty=17.0, degree=1).coef.copy()
    for d in range(2, 6):
        for j in range(d + 1):
            coef[:, _slot(d - j, j)] = r.choice([-1.0, 1.0], 2) * r.uniform(0.5, 1.0, 2) * 0.003 * 23.0 ** (1 - d)
    coef[0, 2] += 0.01                                   # (the rotation's own entries are non-zero already)
    return case([frame(103, 41, 45)], [PolyMap(coef, 5, (22.0, 20.0))], weights=[weight(103, 41, 45)])


def mirrored():
    return case([frame(104, 38, 47)], [distorted(38, 47, deg=-8.0, scale=1.0, tx=35.0, ty=18.0, mirror=True)],
                weights=[weight(104, 38, 47)])


def mixed():
    """one [6] entry, two PolyMaps of different degree and centre, different shapes, one frame inactive, one that
    misses the output; the output's right-hand end is reached by no frame"""
    frames = [frame(105, 24, 31), frame(106, 40, 48), frame(107, 33, 29), frame(108, 12, 14), frame(109, 9, 11)]
    maps = [rot(4.0, tx=4.4, ty=3.3, about=(15, 12)),
            distorted(40, 48, deg=10.0, scale=0.6, tx=30.0, ty=20.0, k=4.0e-5).about((3.0, -2.0)),
            distorted(33, 29, deg=-30.0, scale=1.0, tx=22.0, ty=12.0, degree=2),
            distorted(12, 14, deg=0.0, scale=1.0, tx=20.0, ty=20.0, degree=2),
            distorted(9, 11, deg=5.0, scale=1.0, tx=400.0, ty=10.0, degree=2)]
    return case(frames, maps, out_shape=(37, 90), weights=[weight(105, 24, 31), None, weight(107, 33, 29), None, None],
                active=[1, 1, 1, 0, 1], fill=-3.0)


def many_frames():
    """K = 33 tiny frames: two ctx planes"""
    r = np.random.RandomState(5)
    maps = [distorted(8, 8, deg=r.uniform(-20, 20), scale=1.0, tx=r.uniform(4, 66), ty=r.uniform(4, 33), k=0.0,
                      q=(2e-3, -1e-3), degree=2) for _ in range(33)]
    return case([frame(130 + k, 8, 8) for k in range(33)], maps, weights=[weight(130 + k, 8, 8) for k in range(33)])


def shrink_map(scale):
    return distorted(40, 48, deg=0.0, scale=scale, tx=30.0, ty=18.0, k=2.0e-5, q=(2e-5, -1e-5))


def shrink():
    """a shrinking distorted map whose packed window is 7 or 8 wide"""
    return case([frame(110, 40, 48)], [shrink_map(0.2)], weights=[weight(110, 40, 48)])


def too_small():
    return dict(shrink(), maps=[shrink_map(0.15)])


def folded():
    """X = u - 0.05 u^2: dX/du changes sign at u = 10, inside the frame"""
    from subpixal_amd.resample import PolyMap
    coef = np.zeros((2, 21))
    coef[0, :3] = 30.0, 1.0, 0.0
    coef[1, :3] = 18.0, 0.0, 1.0
    coef[0, _slot(2, 0)] = -0.05
    return dict(shrink(), maps=[PolyMap(coef, 2, (23.5, 19.5))])


FAR = (2000.0, -1500.0)


def far_centre():
    """radial3's map given about a centre 2000 px away"""
    c = radial3()
    return dict(c, maps=[c['maps'][0].about(FAR)])


ALL = dict(degree1=degree1, radial3=radial3, radial3_p06=radial3_p06, radial3_turbo=radial3_turbo,
           radial3_point=radial3_point, degree5=degree5, mirrored=mirrored, mixed=mixed, many_frames=many_frames,
           shrink=shrink, far_centre=far_centre)
# the three the device is compared with the CPU harness on, bit for bit
BITWISE = ('radial3', 'degree5', 'mixed')
