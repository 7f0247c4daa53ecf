"""The drizzle without a GPU: the kernel of subpixal_amd/csrc/spx_drizzle_kernels.h on CPU threads
(tests/cpu_emu/emu_drizzle.cpp, rows packed and launched as spx_capi.hip does) against the numpy scatter of
tests/drizzle_statement.py on every case of tests/drizzle_cases.py, in float32 and float64; exact results where the
arithmetic is dyadic; flux conservation; grid independence; every argument check of the new C entries; the
ValueErrors of `resample.DeviceDrizzle` and the name bookkeeping of `fast_replace_image`."""
import ctypes
import os
import re

import numpy as np
import pytest

import drizzle_cases as dc
import drizzle_emu as de
import drizzle_statement as ds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('spx_drizzle_rows', 'spx_drizzle_f32', 'spx_drizzle_f64')
E_ARG, E_SHAPE = -1, -2
DTYPES = (np.float32, np.float64)


@pytest.fixture(scope='module')
def emuz(tmp_path_factory):
    return de.load(tmp_path_factory)


def both(lib, name, dtype, **kw):
    c = dc.ALL[name]()
    st = de.statement(name, c)
    out = de.run(lib, c, dtype, **kw)
    ds.check(*out, st, what='%s %s' % (name, np.dtype(dtype).name))
    return c, st, out


# ---------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', sorted(dc.ALL))
def test_case_against_the_statement(emuz, name, dtype):
    both(emuz, name, dtype)


def test_the_cases_cover_what_they_claim():
    for name, fn in dc.ALL.items():
        c = fn()
        assert all(5 <= f.shape[0] <= 24 and 7 <= f.shape[1] <= 31 for f in c['frames']), name
        assert c['out_shape'][0] % 8 and c['out_shape'][1] % 32, name
    st = de.statement('pixfrac_tenth', dc.pixfrac_tenth())
    assert st['filled'].mean() > 0.5
    assert not de.statement('misses', dc.misses())['aw'][0].any()
    assert len(dc.many_frames()['frames']) == 33
    assert de.statement('half_outside', dc.half_outside())['aw'][0, 0, 0] > 0


@pytest.mark.parametrize('dtype', DTYPES)
def test_identity_is_exact(emuz, dtype):
    c, st, (sci, wht, ctx) = both(emuz, 'identity_full', dtype)
    d, w = c['frames'][0].astype(dtype), c['weights'][0].astype(np.float32)
    assert np.array_equal(sci, d) and np.array_equal(wht, w) and np.array_equal(ctx[0], (w > 0).astype(np.int32))
    c, st, (sci, wht, ctx) = both(emuz, 'identity', dtype)
    ny, nx = c['frames'][0].shape
    assert np.array_equal(sci[:ny, :nx], c['frames'][0].astype(dtype))
    assert np.array_equal(wht[:ny, :nx], c['weights'][0].astype(np.float32))
    inside = np.zeros(c['out_shape'], bool)
    inside[:ny, :nx] = True
    assert np.all(sci[~inside] == 0) and np.all(wht[~inside] == 0) and np.array_equal(ctx[0], inside.astype(np.int32))


@pytest.mark.parametrize('dtype', DTYPES)
def test_integer_shifts_are_exact(emuz, dtype):
    c, st, (sci, wht, ctx) = both(emuz, 'integer_shifts', dtype)
    seen = np.zeros(c['out_shape'], np.int32)
    for k, (f, w, m) in enumerate(zip(c['frames'], c['weights'], c['maps'])):
        ny, nx = f.shape
        x0, y0 = int(m[2]), int(m[5])
        assert np.array_equal(sci[y0:y0 + ny, x0:x0 + nx], f.astype(dtype))
        assert np.array_equal(wht[y0:y0 + ny, x0:x0 + nx], w.astype(np.float32))
        seen[y0:y0 + ny, x0:x0 + nx] |= 1 << k
    assert np.array_equal(ctx[0], seen) and np.all(wht[seen == 0] == 0)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['twice', 'twice_half_drop'])
def test_a_quarter_on_four_pixels(emuz, name, dtype):
    """A = 2 I: with pixfrac 1 the drop is four whole output pixels, with pixfrac 1/2 it is a quarter of each of
    them; either way a = 1/4 on the same four pixels and nothing anywhere else"""
    c, st, (sci, wht, ctx) = both(emuz, name, dtype)
    f = c['frames'][0]
    ny, nx = f.shape
    exp_w = np.zeros(c['out_shape'])
    exp_s = np.zeros(c['out_shape'])
    for j in range(ny):
        for i in range(nx):
            for Y in (2 * j + 3, 2 * j + 4):
                for X in (2 * i + 2, 2 * i + 3):
                    if Y < c['out_shape'][0] and X < c['out_shape'][1]:
                        exp_w[Y, X] = 0.25
                        exp_s[Y, X] = f[j, i]
    assert np.array_equal(wht, exp_w.astype(np.float32)) and np.array_equal(sci, exp_s.astype(dtype))
    assert np.array_equal(ctx[0], (exp_w > 0).astype(np.int32))


@pytest.mark.parametrize('name', ['rot30', 'rot_tiny', 'mirrored', 'shrink', 'twice_half_drop', 'masked', 'turbo'])
def test_flux_is_conserved(emuz, name):
    """every drop of these cases lies wholly inside the output, and the a of one drop sum to 1: sum(wht) = sum(w).
    The kernel's wht is within bwht of the truth per pixel, the float32 output rounds each by 2^-24, and the sums
    here add n numbers."""
    c, st, (sci, wht, ctx) = both(emuz, name, np.float64)
    total = 0.0
    for k, f in enumerate(c['frames']):
        w = ds.effective_weight(f, None if c['weights'] is None else c['weights'][k],
                                None if c['masks'] is None else c['masks'][k])
        ny, nx = f.shape
        m = c['maps'][k]
        for x, y in ((-0.5, -0.5), (nx - 0.5, -0.5), (-0.5, ny - 0.5), (nx - 0.5, ny - 0.5)):
            X, Y = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
            assert -0.5 <= X <= c['out_shape'][1] - 0.5 and -0.5 <= Y <= c['out_shape'][0] - 0.5, name
        total += w.sum()
    got = wht.astype(np.float64).sum()
    bound = st['bwht'].sum() + 2.0 ** -24 * total + 2 * wht.size * ds.EPS * total
    print('%s: sum wht %.12g, sum w %.12g, bound %.3g' % (name, got, total, bound))
    assert abs(got - total) <= bound


@pytest.mark.parametrize('dtype', DTYPES)
def test_grid_size_does_not_matter_and_runs_are_identical(emuz, dtype):
    for name in ('many_frames', 'mixed_shapes', 'half_outside'):
        c = dc.ALL[name]()
        runs = [de.run(emuz, c, dtype, grid=g) for g in (0, 1, 3, 0)]
        for r in runs[1:]:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(r, runs[0])), name


def test_nothing_is_written_beyond_the_outputs(emuz):
    """the output arrays are exactly as large as the entries ask: every element is written (no -77 is left)"""
    for name in ('misses', 'small_frame', 'many_frames'):
        sci, wht, ctx = de.run(emuz, dc.ALL[name](), np.float32)
        assert not (sci == -77).any() and not (wht == -77).any() and not (ctx == -77).any(), name


def test_the_harness_refuses_what_the_packing_refuses(emuz):
    c = dc.identity()
    for m, rc in (([1, 0, 0, 2, 0, 0], 2), ([0, 0, 0, 0, 0, 0], 2), ([np.nan, 0, 0, 0, 1, 0], 1),
                  ([1, 0, np.inf, 0, 1, 0], 1), ([0.15, 0, 0, 0, 0.15, 0], 3), ([1, 0, 0, 0, 0.125, 0], 3)):
        de.run(emuz, dict(c, maps=[np.array(m, np.float64)]), np.float32, expect=rc)
    de.run(emuz, dict(c, maps=[np.array([0.2, 0, 0, 0, 0.2, 0])]), np.float32)           # window 7 x 7: accepted


# ---------------------------------------------------------------------------------------------------------------
# the boundary
# ---------------------------------------------------------------------------------------------------------------
def _declared():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'subpixal_hip.h')).read(), flags=re.S)
    return set(re.findall(r'\b(spx_[a-z0-9_]+)\s*\(', text))


def test_new_entries_exported_and_declared():
    from subpixal_amd import _ffi, resample
    lib = _ffi.load()
    declared = _declared()
    for name in NEW:
        assert name in declared and name in _ffi.EXPORTED_SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    assert declared == set(_ffi.EXPORTED_SYMBOLS)
    assert lib.spx_abi_version() == _ffi.ABI_VERSION == 4
    header = open(os.path.join(ROOT, 'include', 'subpixal_hip.h')).read()
    assert '#define SPX_DRIZZLE_ROW_BYTES 224' in header and _ffi.DRIZZLE_ROW_BYTES == 224
    for k, v in resample.KERNELS.items():
        assert '#define SPX_DRIZZLE_%s %d' % (k.upper(), v) in header and ds.KERNELS[k] == v
    table = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in ('spx_drizzle_rows', 'spx_drizzle_f32', '_f64'):
        assert '`%s`' % name in table, name


def _tables(K=2, ny=8, nx=9):
    buf = np.zeros(1024, np.float64)
    frames = np.full(K, buf.ctypes.data, np.uint64)
    shapes = np.tile(np.array([ny, nx], np.int32), (K, 1))
    maps = np.tile(np.array([1.0, 0, 0, 0, 1, 0]), (K, 1))
    return buf, frames, shapes, maps


def test_c_argument_errors_of_the_row_packing():
    from subpixal_amd import _ffi
    lib = _ffi.load()
    buf, frames, shapes, maps = _tables()
    rows = np.zeros((2, 224), np.uint8)

    def call(frames=frames, weights=None, masks=None, shapes=shapes, maps=maps, active=None, K=2, pixfrac=1.0,
             kernel=0, ny=37, nx=53, out=rows):
        p = [None if a is None else a.ctypes.data for a in (frames, weights, masks, shapes, maps, active)]
        return lib.spx_drizzle_rows(*p, K, pixfrac, kernel, ny, nx, None if out is None else out.ctypes.data)

    for kw in (dict(K=0), dict(K=129), dict(K=-1), dict(pixfrac=0.0), dict(pixfrac=1.0000001), dict(pixfrac=-0.5),
               dict(pixfrac=float('nan')), dict(kernel=3), dict(kernel=-1), dict(frames=None), dict(shapes=None),
               dict(maps=None), dict(out=None), dict(frames=np.array([frames[0], 0], np.uint64))):
        assert call(**kw) == E_ARG, kw
        assert lib.spx_last_error()
    assert b'null' in lib.spx_last_error()
    for bad in ([1, 0, 0, 2, 0, 0], [0, 0, 0, 0, 0, 0], [1e-300, 0, 0, 0, 1e-300, 0]):
        assert call(maps=np.array([maps[0], bad], np.float64)) == E_ARG and b'singular' in lib.spx_last_error(), bad
    for bad in ([np.nan, 0, 0, 0, 1, 0], [1, 0, np.inf, 0, 1, 0], [1, 0, 0, 0, 1, -np.inf]):
        assert call(maps=np.array([maps[0], bad], np.float64)) == E_ARG and b'finite' in lib.spx_last_error(), bad
    for kw in (dict(ny=0), dict(nx=0), dict(ny=65536, nx=32768), dict(shapes=np.array([[8, 9], [0, 9]], np.int32)),
               dict(shapes=np.array([[8, 9], [65536, 32768]], np.int32)),
               dict(maps=np.array([maps[0], [0.15, 0, 0, 0, 0.15, 0]])),             # rx = 0.575 / 0.15 = 3.83: 9 wide
               dict(maps=np.array([maps[0], [1, 0, 0, 0, 0.125, 0]]))):
        assert call(**kw) == E_SHAPE, kw
    assert b'8 x 8' in lib.spx_last_error()
    assert not rows.any()                                       # nothing is written on an error
    assert call(K=1) == 0 and rows[0].any() and not rows[1].any()
    assert call(weights=np.zeros(2, np.uint64), masks=np.zeros(2, np.uint64), active=np.array([1, 0], np.uint8)) == 0
    # the row is the documented layout: pointers, shape, flag, map
    r = rows[1].view(np.uint64)
    assert r[0] == buf.ctypes.data and r[1] == 0 and r[2] == 0
    assert list(rows[1, 24:40].view(np.int32)) == [8, 9, 0, 0] and list(rows[0, 24:40].view(np.int32)) == [8, 9, 1, 0]
    assert list(rows[1, 40:88].view(np.float64)) == [1.0, 0, 0, 0, 1, 0]


def test_c_argument_errors_of_the_launch_before_any_hip_call():
    from subpixal_amd import _ffi
    lib = _ffi.load()
    buf = np.zeros(64, np.float64)
    b = buf.ctypes.data
    for fn in (lib.spx_drizzle_f32, lib.spx_drizzle_f64):
        def call(rows=b, K=2, kernel=0, ny=4, nx=4, sci=b, wht=b, ctx=b):
            return fn(rows, K, kernel, 0.0, ny, nx, sci, wht, ctx, None)
        for name in ('rows', 'sci', 'wht', 'ctx'):
            assert call(**{name: None}) == E_ARG and b'null' in lib.spx_last_error(), name
        for kw in (dict(K=0), dict(K=129), dict(kernel=3), dict(kernel=-1)):
            assert call(**kw) == E_ARG, kw
        for kw in (dict(ny=0), dict(nx=-1), dict(ny=65536, nx=32768)):
            assert call(**kw) == E_SHAPE, kw
    assert not buf.any()


def _host_drizzle(K=3, **kw):
    from subpixal_amd import resample
    frames = [np.zeros((6, 7), np.float32) for _ in range(K)]
    a = dict(frames=frames, maps=np.tile([1.0, 0, 0, 0, 1, 0], (K, 1)), out_shape=(9, 10),
             names=['a', 'b', 'c', 'd', 'e'][:K])
    a.update(kw)
    return resample.DeviceDrizzle(**a)


def test_python_argument_errors_before_the_device():
    f = np.zeros((6, 7), np.float32)
    for kw, what in ((dict(frames=[]), 'frames'), (dict(frames=129 * [f], maps=np.zeros((129, 6)), names=None), 'frames'),
                     (dict(frames=[f, f, f.astype(np.float64)]), 'frames'), (dict(frames=[f, f, np.zeros(7, np.float32)]), 'frames'),
                     (dict(frames=[f.astype(np.int32)] * 3), 'dtype'), (dict(names=['a', 'a', 'b']), 'names'),
                     (dict(names=['a', 'b']), 'names'), (dict(maps=np.zeros((3, 5))), 'maps'),
                     (dict(maps=np.tile([1.0, 0, 0, 2, 0, 0], (3, 1))), 'singular'),
                     (dict(maps=np.tile([1.0, 0, np.nan, 0, 1, 0], (3, 1))), 'finite'),
                     (dict(weights=[None, None]), 'weights'), (dict(weights=[None, np.zeros((6, 6), np.float32), None]), 'weights'),
                     (dict(masks=[np.zeros((7, 6), bool), None, None]), 'masks'), (dict(out_shape=(0, 5)), 'out_shape'),
                     (dict(out_shape=(5,)), 'out_shape'), (dict(pixfrac=0.0), 'pixfrac'), (dict(pixfrac=1.5), 'pixfrac'),
                     (dict(kernel='gaussian'), 'kernel')):
        with pytest.raises(ValueError, match=what):
            _host_drizzle(**kw)
    d = _host_drizzle()
    assert d.reference_image == (9, 10) and d.output_crclean is None and d.output_sci is None
    assert d.dtype == np.float32
    with pytest.raises(ValueError, match='singular'):
        d.set_map('a', [0, 0, 0, 0, 0, 0])
    with pytest.raises(ValueError, match='no frame'):
        d.set_map('z', [1, 0, 0, 0, 1, 0])
    with pytest.raises(ValueError, match='kernel'):
        d.set_config_parameters(kernel='lanczos3')
    d.set_map('b', [1, 0, 2.5, 0, 1, -1])
    assert list(d.map('b')) == [1, 0, 2.5, 0, 1, -1] and list(d.map('a')) == [1, 0, 0, 0, 1, 0]
    d.map('b')[2] = 9
    assert d.map('b')[2] == 2.5


def test_fast_replace_image_keeps_the_list_as_the_reference_does():
    d = _host_drizzle(K=4)
    runs = []
    d.execute = lambda: runs.append(list(d.input_image_names))          # no device here: the list is the subject
    d.fast_replace_image(None, None)                                      # both None: nothing happens
    d.fast_replace_image('b', 'b')                                        # the same image: nothing happens
    assert runs == [] and d.input_image_names == ['a', 'b', 'c', 'd']
    d.fast_replace_image('b', None)
    assert d.input_image_names == ['a', 'c', 'd'] and d.table_names == ['a', 'b', 'c', 'd']
    d.fast_replace_image('b', None)                                       # not in the list: nothing is dropped
    assert d.input_image_names == ['a', 'c', 'd']
    d.fast_replace_image(None, 'c')                                       # in the list already: not added
    assert d.input_image_names == ['a', 'c', 'd'] and d.table_names == ['a', 'b', 'c', 'd']
    d.fast_replace_image('c', 'b')                                        # the added image goes to the END
    assert d.input_image_names == ['a', 'd', 'b'] and d.table_names == ['a', 'c', 'd', 'b']
    d.fast_add_image('c')
    assert d.input_image_names == ['a', 'd', 'b', 'c']
    d.fast_drop_image('a')
    assert d.input_image_names == ['d', 'b', 'c']
    assert runs == [['a', 'c', 'd'], ['a', 'c', 'd'], ['a', 'c', 'd'], ['a', 'd', 'b'], ['a', 'd', 'b', 'c'],
                    ['d', 'b', 'c']]                                      # every call that got past the two returns ran
    with pytest.raises(ValueError, match='was ever given'):
        d.fast_add_image('zz')
    # a copy has its own list and maps and shares the frames
    q = d.copy()
    q.execute = lambda: None
    q.fast_drop_image('d')
    q.set_map('b', [1, 0, 7, 0, 1, 7])
    assert d.input_image_names == ['d', 'b', 'c'] and q.input_image_names == ['b', 'c']
    assert d.map('b')[2] == 0 and q.map('b')[2] == 7 and q._pool['b'] is d._pool['b']
