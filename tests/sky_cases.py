"""Cases of the whole-frame sigma-clipped statistics for tests/test_sky_cpu.py (kernels on CPU threads) and
tests/test_gpu_sky.py (the device).  Every builder takes the dtype and returns
``dict(frames, weights, masks, lower, upper, lsigma, usigma, max_iters, stat)`` (weights / masks: None or one entry
per frame); COVERS names what the case is there for, as a predicate over the statement's results that
test_every_case_covers_what_it_names asserts.  Frames are at most 101 x 61 pixels with odd sides.  Not a test module."""
import numpy as np

F32, F64 = np.float32, np.float64
ALL, COVERS, ONLY = {}, {}, {}


def case(covers, only=None):
    def deco(fn):
        name = fn.__name__
        ALL[name] = fn
        COVERS[name] = covers
        if only is not None:
            ONLY[name] = np.dtype(only)
        return fn
    return deco


def dtypes(name):
    return (ONLY[name],) if name in ONLY else (np.dtype(F32), np.dtype(F64))


def make(frames, weights=None, masks=None, lower=None, upper=None, lsigma=4.0, usigma=4.0, max_iters=5, stat='median'):
    return dict(frames=frames, weights=weights, masks=masks, lower=lower, upper=upper, lsigma=lsigma, usigma=usigma,
                max_iters=max_iters, stat=stat)


def noise(seed, ny, nx, dtype, level=100.0, sigma=3.0):
    r = np.random.RandomState(seed)
    return (level + sigma * r.standard_normal((ny, nx))).astype(dtype)


def with_sources(a, seed, nsrc, peak):
    r = np.random.RandomState(seed)
    ny, nx = a.shape
    yy, xx = np.mgrid[:ny, :nx]
    out = a.astype(np.float64)
    for _ in range(nsrc):
        y, x, s = r.uniform(0, ny), r.uniform(0, nx), r.uniform(1.0, 2.5)
        out += peak * r.uniform(0.3, 1.0) * np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2 * s * s))
    return out.astype(a.dtype)


@case(lambda st: st[0]['rounds'] >= 3 and st[0]['n_final'] < st[0]['n_usable'])
def noise_and_sources(dt):
    return make([with_sources(noise(1, 45, 67, dt), 2, 12, 400.0)], lsigma=3.0, usigma=3.0)


@case(lambda st: st[0]['n_final'] % 2 == 1)
def odd_count(dt):
    return make([noise(3, 7, 9, dt)], max_iters=0)


@case(lambda st: st[0]['n_final'] % 2 == 0 and st[0]['n_final'] == 62)
def even_count(dt):
    m = np.zeros((7, 9), np.uint8)
    m[3, 4] = 1
    return make([noise(4, 7, 9, dt)], masks=[m], max_iters=0)


@case(lambda st: st[0]['n_usable'] == 1 and st[0]['std'] == 0 and st[0]['med'] == 42.5)
def one_pixel(dt):
    return make([np.array([[42.5]], dt)], max_iters=1)


@case(lambda st: st[0]['n_usable'] == 2 and st[0]['med'] == 2.0 and st[0]['std'] == 1.0)
def two_pixels(dt):
    return make([np.array([[1.0, 3.0]], dt)], max_iters=1)


@case(lambda st: st[0]['std'] == 0 and st[0]['rounds'] == 1 and st[0]['mean'] == 7.25)
def constant_frame(dt):
    return make([np.full((21, 33), 7.25, dt)], max_iters=2)


@case(lambda st: st[0]['med'] == 1.5 and st[0]['n_final'] == 62)
def two_valued_straddle(dt):
    a = np.where(np.arange(63).reshape(7, 9) % 2 == 0, 1.0, 2.0).astype(dt)
    m = np.zeros((7, 9), np.uint8)
    m[0, 0] = 1                                                    # 31 ones and 31 twos stay
    return make([a], masks=[m], stat='mode', max_iters=2)


@case(lambda st: st[0]['med'] == 0.0 and st[0]['n_final'] == 99)
def signed_zeros(dt):
    r = np.random.RandomState(5)
    a = r.choice(np.array([-1.0, -0.0, 0.0, 0.0, -0.0, 1.0]), size=(9, 11)).astype(dt)
    a[0, :4] = (-2.0, -0.0, 0.0, 2.0)
    return make([a], max_iters=1)


@case(lambda st: st[0]['rounds'] == 2 and 1e37 < st[0]['hi'] < 3e38 and st[0]['n_final'] == st[0]['n_usable'] - 6)
def denormals_and_outliers(dt):
    # multiples of 1e-40: denormal in float32 (normal in float64, where the same numbers are used)
    r = np.random.RandomState(6)
    a = (r.randint(-3000, 3000, size=(9, 13)) * 1e-40).astype(dt)
    a[0, :3] = 3e38
    a[8, :3] = -3e38
    return make([a], lsigma=3.0, usigma=3.0, max_iters=2)


@case(lambda st: st[0]['n_usable'] == 15 * 11 - 6 - 15 - 10 and st[0]['status'] == 0)
def nonfinite_mask_weights(dt):
    a = noise(7, 11, 15, dt)
    a[0, 0], a[0, 1], a[0, 2] = np.nan, np.inf, -np.inf
    m = np.zeros(a.shape, np.uint8)
    m[5, :] = 1
    m[5, 3] = 200
    w = np.ones(a.shape, dt)
    w[1, :4] = 0.0
    w[2, :3] = -1.0
    w[3, :3] = np.nan
    a[10, 0:3] = np.nan
    w[10, 0] = 0.0                                                  # a NaN pixel whose weight is zero too
    m[5, 0:2] = 1
    return make([a], weights=[w], masks=[m], max_iters=2, lsigma=3.0, usigma=3.0)


@case(lambda st: st[0]['lo'] >= 95.0 and st[0]['hi'] <= 104.0 and st[0]['n_usable'] < 45 * 33)
def hard_bounds(dt):
    return make([noise(8, 33, 45, dt)], lower=95.0, upper=104.0, max_iters=1)


@case(lambda st: st[0]['status'] == 1 and st[0]['n_usable'] == 0 and np.isnan(st[0]['med']))
def bounds_leave_nothing(dt):
    return make([noise(9, 5, 7, dt)], lower=500.0, upper=600.0, max_iters=1)


@case(lambda st: st[0]['rounds'] >= 2 and abs((st[0]['med'] - st[0]['lo']) - (st[0]['hi'] - st[0]['med'])) > 1.0)
def asymmetric_factors(dt):
    return make([with_sources(noise(10, 33, 45, dt), 11, 5, 200.0)], lsigma=2.0, usigma=3.5, max_iters=3)


@case(lambda st: st[0]['rounds'] == 1 and st[0]['n_final'] == st[0]['n_usable'] and np.isinf(st[0]['hi']))
def no_iterations(dt):
    return make([with_sources(noise(12, 21, 33, dt), 13, 4, 300.0)], max_iters=0, stat='mean')


@case(lambda st: st[0]['rounds'] == 1 and st[0]['n_final'] == 62 and np.isinf(st[0]['lo']) and st[0]['std'] == 0.5)
def factors_below_one_would_empty(dt):
    c = two_valued_straddle(dt)
    c.update(lsigma=0.01, usigma=0.01, stat='median')
    return c


@case(lambda st: st[0]['sky'] == st[0]['mean'] != st[0]['med'])
def stat_mean(dt):
    return make([noise(14, 21, 33, dt)], stat='mean', max_iters=2, lsigma=3.0, usigma=3.0)


@case(lambda st: abs(st[0]['mean'] - st[0]['med']) < 0.25 * st[0]['std'] and st[0]['sky'] != st[0]['med'])
def stat_mode_near(dt):
    return make([noise(15, 21, 33, dt)], stat='mode', max_iters=2, lsigma=3.0, usigma=3.0)


@case(lambda st: abs(st[0]['mean'] - st[0]['med']) > 0.35 * st[0]['std'] > 0 and st[0]['sky'] == st[0]['med'])
def stat_mode_far(dt):
    r = np.random.RandomState(16)
    a = 0.01 * r.standard_normal((21, 33))
    a[r.uniform(size=a.shape) < 0.4] += 1.0
    return make([a.astype(dt)], stat='mode', max_iters=0)


@case(lambda st: 1.0 < st[0]['med'] < 1.0 + 2.0 ** -20 and st[0]['std'] < 2.0 ** -20, only=F32)
def low_key_bits_f32(dt):
    r = np.random.RandomState(17)
    a = (1.0 + r.randint(0, 8, size=(9, 11)) * 2.0 ** -23).astype(dt)
    return make([a], max_iters=0)


@case(lambda st: 1.0 < st[0]['med'] < 1.0 + 2.0 ** -48 and 0 < st[0]['std'] < 2.0 ** -48, only=F64)
def low_word_f64(dt):
    # 1 + k 2^-52: the keys differ only in the low word, so the selection walks every digit
    r = np.random.RandomState(18)
    a = 1.0 + r.randint(0, 16, size=(9, 11)) * 2.0 ** -52
    return make([a.astype(dt)], max_iters=0)


@case(lambda st: len(st) == 5 and st[1]['status'] == 1 and st[3]['n_usable'] == 1 and st[0]['rounds'] >= 2)
def batch_of_five(dt):
    f = [with_sources(noise(19, 21, 33, dt), 20, 3, 300.0), noise(21, 5, 7, dt), noise(22, 13, 9, dt, level=-5.0),
         np.array([[3.5]], dt), noise(23, 31, 3, dt, level=1e4, sigma=30.0)]
    masks = [None, np.ones((5, 7), np.uint8), None, None, None]
    w = np.ones((13, 9), dt)
    w[::2] = 0.0
    return make(f, weights=[None, None, w, None, None], masks=masks, max_iters=2, lsigma=2.5, usigma=2.5, stat='mode')


@case(lambda st: st[0]['n_usable'] == 101 * 61 > 4096)
def thread_takes_two_pixels(dt):
    return make([noise(24, 61, 101, dt)], max_iters=1, lsigma=3.0, usigma=3.0)


@case(lambda st: st[0]['n_usable'] == 15)
def most_workgroups_idle(dt):
    return make([noise(25, 3, 5, dt)], max_iters=1, lsigma=1.5, usigma=1.5)
