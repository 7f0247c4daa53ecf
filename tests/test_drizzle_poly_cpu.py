"""The drizzle through polynomial maps without a GPU: the kernel of subpixal_amd/csrc/spx_drizzle_poly_kernels.h on CPU
threads (tests/cpu_emu/emu_drizzle_poly.cpp, rows packed and launched as spx_capi.hip does) against the numpy scatter
of tests/drizzle_poly_statement.py on every case of tests/drizzle_poly_cases.py, in float32 and float64; the degree-1
case against the affine kernel; grid independence; sentinels; partition of unity; what the packing refuses; the
argument checks of the new C entries; the algebra of `resample.PolyMap`; `align.compose_fit`; the ValueErrors of
`resample.DeviceDrizzle` for polynomial maps."""
import os
import re

import numpy as np
import pytest

import drizzle_emu as de
import drizzle_poly_cases as pc
import drizzle_poly_emu as pe
import drizzle_poly_statement as dps
import drizzle_statement as ds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('spx_drizzle_poly_rows', 'spx_drizzle_poly_f32', 'spx_drizzle_poly_f64')
E_ARG, E_SHAPE = -1, -2
DTYPES = (np.float32, np.float64)


@pytest.fixture(scope='module')
def emuzp(tmp_path_factory):
    return pe.load(tmp_path_factory)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', sorted(pc.ALL))
def test_case_against_the_statement(emuzp, name, dtype):
    c = pc.ALL[name]()
    r = dps.check(*pe.run(emuzp, c, dtype), pe.statement(name, c), what='%s %s' % (name, np.dtype(dtype).name))
    print(name, np.dtype(dtype).name, r)


@pytest.mark.parametrize('name', sorted(pc.ALL))
def test_the_statement_alone_stays_inside_the_caps_of_check(name):
    """the two caps are conditions on the cases: pixels too faint to compare <= 1 %, grey ctx pairs < 1 %"""
    st = pe.statement(name, pc.ALL[name]())
    faint = (~(st['wht'] > 2.0 * st['bwht']) & ~st['filled']).sum()
    grey = (~(st['aw'] > 1e-9 * st['wmax']) & ~(st['aw'] == 0.0)).sum()
    assert faint <= 0.01 * st['wht'].size and grey < 0.01 * st['aw'].size, (name, faint, grey)


def test_the_cases_cover_what_they_claim():
    for name, fn in pc.ALL.items():
        c = fn()
        assert c['out_shape'][0] % 8 and c['out_shape'][1] % 32 and c['out_shape'][1] > 64 and c['out_shape'][0] > 16
    m = pc.radial3()['maps'][0]
    yy, xx = np.mgrid[0:40, 0:48].astype(np.float64)
    j = m.jacobian(xx, yy)
    det = j[..., 0, 0] * j[..., 1, 1] - j[..., 0, 1] * j[..., 1, 0]
    assert det.max() / det.min() > 1.18                        # +-10 % area change across the frame
    assert np.all(pc.degree5()['maps'][0].coef != 0.0)
    jm = pc.mirrored()['maps'][0].jacobian(xx[:38, :47], yy[:38, :47])
    assert np.all(jm[..., 0, 0] * jm[..., 1, 1] - jm[..., 0, 1] * jm[..., 1, 0] < 0)
    c = pc.mixed()
    st = pe.statement('mixed', c)
    assert not st['aw'][3].any() and not st['aw'][4].any() and st['aw'][0].any() and st['aw'][2].any()
    assert st['filled'][:, 80:].all()                          # a region no frame reaches
    assert len({type(m).__name__ for m in c['maps']}) == 2 and len({f.shape for f in c['frames']}) == 5
    assert len(pc.many_frames()['frames']) == 33
    assert tuple(pc.far_centre()['maps'][0].center) == pc.FAR


@pytest.mark.parametrize('dtype', DTYPES)
def test_a_degree_1_map_agrees_with_the_affine_kernel(emuzp, tmp_path_factory, dtype):
    """within the sum of the two statements' bounds"""
    c, t = pc.degree1(), pc.affine_twin()
    sp, sa = pe.statement('degree1', c), de.statement('poly_affine_twin', t)
    gp = pe.run(emuzp, c, dtype)
    ga = de.run(de.load(tmp_path_factory), t, dtype)
    assert np.array_equal(gp[1] > 0, ga[1] > 0)
    ew = np.abs(gp[1].astype(np.float64) - ga[1])
    assert np.all(ew <= sp['bwht'] + sa['bwht'] + 2.0 ** -23 * sa['wht'])
    ok = (sp['wht'] > 2.0 * sp['bwht']) & (sa['wht'] > 2.0 * sa['bwht'])
    u = 2.0 ** -24 if dtype == np.float32 else ds.EPS
    with np.errstate(invalid='ignore', divide='ignore'):
        bs = sum((s['bnum'] + np.abs(s['sci']) * s['bwht']) / (s['wht'] - s['bwht']) + (ds.EPS + u) * np.abs(s['sci'])
                 for s in (sp, sa))
    es = np.abs(gp[0].astype(np.float64) - ga[0])
    assert np.all(es[ok] <= bs[ok]), es[ok].max()
    assert np.array_equal(gp[2], ga[2])


@pytest.mark.parametrize('dtype', DTYPES)
def test_grid_size_does_not_matter_and_runs_are_identical(emuzp, dtype):
    for name in ('many_frames', 'mixed', 'radial3'):
        c = pc.ALL[name]()
        runs = [pe.run(emuzp, c, dtype, grid=g) for g in (0, 1, 3, 0)]
        for r in runs[1:]:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(r, runs[0])), name


def test_nothing_is_written_beyond_the_outputs(emuzp):
    """three guard rows of sentinel before and after every output, in the same allocation, stay untouched
    (drizzle_poly_emu.run checks them), and every element between them is written: two runs over different sentinels
    agree everywhere"""
    for name in ('mixed', 'many_frames', 'shrink'):
        c = pc.ALL[name]()
        for dtype in DTYPES:
            a = pe.run(emuzp, c, dtype, sentinel=-77.0, guard=3)
            b = pe.run(emuzp, c, dtype, sentinel=55.0, guard=3)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), name


@pytest.mark.parametrize('name', ['radial3', 'degree5', 'mirrored'])
def test_partition_of_unity(emuzp, name):
    """unit data and weights at pixfrac 1 on an output that holds every drop whole: the a of one drop sum to 1 over
    the output pixels, so sum(wht) is the number of input pixels (the kernel's wht is within bwht of the truth per
    pixel, the float32 output rounds each by 2^-24, the sums here add n numbers); sci = 1 wherever anything lands"""
    from subpixal_amd.resample import PolyMap
    c = pc.ALL[name]()
    ny, nx = c['frames'][0].shape
    m = c['maps'][0]
    coef = m.coef.copy()
    coef[:, 0] += 45.0 - np.array(m(0.5 * (nx - 1), 0.5 * (ny - 1)))        # the frame's centre lands on (45, 45)
    m = PolyMap(coef, m.degree, m.center)
    out = (91, 93)
    for x, y in ((-0.5, -0.5), (nx - 0.5, -0.5), (-0.5, ny - 0.5), (nx - 0.5, ny - 0.5)):
        X, Y = m(x, y)
        assert 0.5 <= X <= out[1] - 1.5 and 0.5 <= Y <= out[0] - 1.5
    c = dict(c, frames=[np.ones((ny, nx))], maps=[m], weights=None, masks=None, out_shape=out)
    sci, wht, ctx = pe.run(emuzp, c, np.float64)
    st = dps.statement(c['frames'], c['maps'], out)
    assert np.all(sci[wht > 0] == 1.0)
    got, total = wht.astype(np.float64).sum(), float(ny * nx)
    bound = st['bwht'].sum() + 2.0 ** -24 * total + 2 * wht.size * ds.EPS * total
    print('%s: sum wht %.12g, drops %d, bound %.3g' % (name, got, ny * nx, bound))
    assert abs(got - total) <= bound


def test_the_window_of_the_shrinking_map_and_what_the_packing_refuses(emuzp):
    rc, rows = pe.pack_rows(pc.shrink())
    rx, ry = pe.window(rows[0])
    assert rc == 0 and 7.0 <= 2 * rx + 1 <= 8.0 and 7.0 <= 2 * ry + 1 <= 8.0, (rx, ry)
    from subpixal_amd import _ffi
    lib = _ffi.load()
    rc, rows = pe.pack_rows(pc.too_small())
    assert rc == E_SHAPE and b'8 x 8' in lib.spx_last_error() and not rows.any()
    rc, rows = pe.pack_rows(pc.folded())
    assert rc == E_ARG and b'singular' in lib.spx_last_error() and not rows.any()
    pe.run(emuzp, pc.too_small(), np.float32, expect=3)
    pe.run(emuzp, pc.folded(), np.float32, expect=2)


def _tables(K=2, ny=8, nx=9):
    buf = np.zeros(1024, np.float64)
    frames = np.full(K, buf.ctypes.data, np.uint64)
    shapes = np.tile(np.array([ny, nx], np.int32), (K, 1))
    coef = np.zeros((K, 2, 21))
    coef[:, 0, 1] = coef[:, 1, 2] = 1.0
    return buf, frames, shapes, coef, np.ones(K, np.int32), np.zeros((K, 2))


def test_c_argument_errors_of_the_row_packing():
    from subpixal_amd import _ffi
    lib = _ffi.load()
    buf, frames, shapes, coef, degree, center = _tables()
    rows = np.zeros((2, _ffi.DRIZZLE_POLY_ROW_BYTES), np.uint8)

    def call(frames=frames, weights=None, masks=None, shapes=shapes, coef=coef, degree=degree, center=center,
             active=None, K=2, pixfrac=1.0, kernel=0, ny=37, nx=70, out=rows):
        p = [None if a is None else a.ctypes.data for a in (frames, weights, masks, shapes, coef, degree, center,
                                                             active)]
        return lib.spx_drizzle_poly_rows(*p, K, pixfrac, kernel, ny, nx, None if out is None else out.ctypes.data)

    def with_coef(k, a, slot, v, deg=None):
        c, d = coef.copy(), degree.copy()
        c[k, a, slot] = v
        if deg:
            d[k] = deg
        return dict(coef=c, degree=d)

    for kw in (dict(K=0), dict(K=129), dict(pixfrac=0.0), dict(pixfrac=1.5), dict(pixfrac=float('nan')),
               dict(kernel=3), dict(kernel=-1), dict(frames=None), dict(shapes=None), dict(coef=None),
               dict(degree=None), dict(center=None), dict(out=None),
               dict(frames=np.array([frames[0], 0], np.uint64)), dict(degree=np.array([1, 0], np.int32)),
               dict(degree=np.array([6, 1], np.int32)), with_coef(1, 0, 2, np.nan), with_coef(1, 1, 5, np.inf, deg=2),
               dict(center=np.array([[0, 0], [np.nan, 0]], np.float64)),
               with_coef(1, 0, 1, 0.0), with_coef(1, 0, 3, -0.2, deg=2)):
        assert call(**kw) == E_ARG, kw
        assert lib.spx_last_error()
    assert call(**with_coef(1, 0, 5, np.nan)) == 0            # a slot above the degree is ignored
    rows[:] = 0
    for kw in (dict(ny=0), dict(nx=0), dict(ny=65536, nx=32768), dict(shapes=np.array([[8, 9], [0, 9]], np.int32)),
               dict(coef=coef * 0.15)):
        assert call(**kw) == E_SHAPE, kw
    assert b'8 x 8' in lib.spx_last_error()
    assert not rows.any()                                       # nothing is written on an error
    assert call(K=1) == 0 and rows[0].any() and not rows[1].any()
    assert call(weights=np.zeros(2, np.uint64), masks=np.zeros(2, np.uint64), active=np.array([1, 0], np.uint8)) == 0
    # the first 40 bytes are the affine row's: pointers, shape, flag
    r = rows[1].view(np.uint64)
    assert r[0] == buf.ctypes.data and r[1] == 0 and r[2] == 0
    assert list(rows[1, 24:40].view(np.int32)) == [8, 9, 0, 0] and list(rows[0, 24:40].view(np.int32)) == [8, 9, 1, 0]
    assert list(rows[0, _ffi.DRIZZLE_POLY_ROW_DEGREE:_ffi.DRIZZLE_POLY_ROW_DEGREE + 8].view(np.int32)) == [1, 0]
    assert list(rows[0, _ffi.DRIZZLE_POLY_ROW_CENTER:_ffi.DRIZZLE_POLY_ROW_CENTER + 16].view(np.float64)) == [4.0, 3.5]
    assert list(rows[0, _ffi.DRIZZLE_POLY_ROW_COEF:_ffi.DRIZZLE_POLY_ROW_COEF + 24].view(np.float64)) == [4.0, 1.0, 0.0]
    assert list(rows[0, _ffi.DRIZZLE_POLY_ROW_INV:_ffi.DRIZZLE_POLY_ROW_INV + 32].view(np.float64)) == [1.0, 0, 0, 1.0]
    assert list(rows[0, _ffi.DRIZZLE_POLY_ROW_DROP:_ffi.DRIZZLE_POLY_ROW_DROP + 16].view(np.float64)) == [0.5, 0.5]


def test_c_argument_errors_of_the_launch_before_any_hip_call():
    from subpixal_amd import _ffi
    lib = _ffi.load()
    buf = np.zeros(64, np.float64)
    b = buf.ctypes.data
    for fn in (lib.spx_drizzle_poly_f32, lib.spx_drizzle_poly_f64):
        def call(rows=b, K=2, kernel=0, ny=4, nx=4, sci=b, wht=b, ctx=b):
            return fn(rows, K, kernel, 0.0, ny, nx, sci, wht, ctx, None)
        for name in ('rows', 'sci', 'wht', 'ctx'):
            assert call(**{name: None}) == E_ARG and b'null' in lib.spx_last_error(), name
        for kw in (dict(K=0), dict(K=129), dict(kernel=3), dict(kernel=-1)):
            assert call(**kw) == E_ARG, kw
        for kw in (dict(ny=0), dict(nx=-1), dict(ny=65536, nx=32768)):
            assert call(**kw) == E_SHAPE, kw
    assert not buf.any()


def _declared():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'subpixal_hip.h')).read(), flags=re.S)
    return set(re.findall(r'\b(spx_[a-z0-9_]+)\s*\(', text))


def test_new_entries_exported_and_declared():
    from subpixal_amd import _ffi
    lib = _ffi.load()
    declared = _declared()
    for name in NEW:
        assert name in declared and name in _ffi.EXPORTED_SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    assert declared == set(_ffi.EXPORTED_SYMBOLS)
    assert lib.spx_abi_version() == _ffi.ABI_VERSION == 4
    header = open(os.path.join(ROOT, 'include', 'subpixal_hip.h')).read()
    assert '#define SPX_DRIZZLE_POLY_ROW_BYTES %d' % _ffi.DRIZZLE_POLY_ROW_BYTES in header
    table = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in ('spx_drizzle_poly_rows', 'spx_drizzle_poly_f32'):
        assert '`%s`' % name in table, name


# ---------------------------------------------------------------------------------------------------------------
# PolyMap
# ---------------------------------------------------------------------------------------------------------------
def _points(n=200, seed=3):
    r = np.random.RandomState(seed)
    return r.uniform(-0.5, 47.5, n), r.uniform(-0.5, 39.5, n)


@pytest.mark.parametrize('which', ['radial3', 'degree5', 'mirrored'])
def test_polymap_algebra_at_random_points(which):
    from subpixal_amd.resample import PolyMap
    m = pc.ALL[which]()['maps'][0]
    x, y = _points()
    X, Y = m(x, y)
    size = max(np.abs(X).max(), np.abs(Y).max(), 48.0)
    g = np.array([1.0003, -0.002, 0.31, 0.0015, 0.9998, -0.27])
    gx, gy = g[0] * x + g[1] * y + g[2], g[3] * x + g[4] * y + g[5]
    mg = m.compose(g)
    assert isinstance(mg, PolyMap) and mg.degree == m.degree
    assert np.abs(np.array(mg(x, y)) - np.array(m(gx, gy))).max() <= 1e-12 * size
    for c in ((0.0, 0.0), (100.5, -40.25), tuple(m.center)):
        ma = m.about(c)
        assert tuple(ma.center) == c and np.abs(np.array(ma(x, y)) - np.array([X, Y])).max() <= 1e-12 * size
    xi, yi = m.inverse(X, Y)
    assert max(np.abs(xi - x).max(), np.abs(yi - y).max()) <= 1e-10
    f, res = PolyMap.fit(m, (40, 48), degree=m.degree)
    assert res < 1e-9 and np.abs(np.array(f(x, y)) - np.array([X, Y])).max() < 1e-9
    _, res1 = PolyMap.fit(m, (40, 48), degree=1)
    assert res1 > 1e-2                                          # the residual does report what a fit leaves
    # the Jacobian against central differences, and the linearisation at the centre
    h = 1e-5
    j = m.jacobian(x, y)
    num = (np.array(m(x + h, y)) - np.array(m(x - h, y))) / (2 * h)
    assert np.abs(j[:, :, 0].T - num).max() < 1e-8
    a = m.affine()
    xc, yc = m.center
    assert np.allclose([a[0] * xc + a[1] * yc + a[2], a[3] * xc + a[4] * yc + a[5]], m(xc, yc), rtol=0, atol=1e-12 * size)
    assert np.allclose(a[[0, 1, 3, 4]], m.jacobian(xc, yc).ravel(), rtol=0, atol=1e-15)


def test_polymap_is_a_checked_immutable_value():
    from subpixal_amd.resample import PolyMap
    m = PolyMap.from_affine([1.0, 0.1, 2.0, -0.1, 1.0, 3.0], (5.0, 6.0))
    assert m.degree == 1 and np.allclose(m(np.array([7.0]), np.array([8.0])), ([9.8], [10.3]))
    assert np.allclose(m.affine(), [1.0, 0.1, 2.0, -0.1, 1.0, 3.0])
    with pytest.raises(AttributeError):
        m.degree = 2
    with pytest.raises(ValueError):
        m.coef[0, 0] = 1.0
    for kw in (dict(degree=0), dict(degree=6), dict(degree=1.5), dict(coef=np.zeros((2, 2))), dict(coef=np.zeros(21)),
               dict(coef=np.full((2, 21), np.nan)), dict(center=(np.inf, 0))):
        a = dict(coef=np.zeros((2, 21)), degree=2, center=(0.0, 0.0))
        a.update(kw)
        with pytest.raises(ValueError, match='maps'):
            PolyMap(**a)
    c = np.ones((2, 21))
    assert not PolyMap(c, 2).coef[:, 6:].any()                  # slots above the degree are cleared
    inv = PolyMap(np.array([[0.0, 1.0, 0.0, 5.0], [0.0, 0.0, 1.0, 0.0]])[:, :3], 1)
    with pytest.raises(ValueError, match='converge'):
        pc.folded()['maps'][0].inverse(np.array([500.0]), np.array([0.0]))
    assert inv.inverse(1.0, 2.0)[0] == 1.0


def test_compose_fit_keeps_affine_maps_to_the_bit_and_composes_polynomials():
    from subpixal_amd import align
    from subpixal_amd.resample import PolyMap
    fit = dict(fit_matrix=np.array([[1.00002, -3.1e-5], [2.9e-5, 0.99997]]), offset=np.array([0.21, -0.13]),
               center=np.array([192.0, 190.0]))
    m = np.array([0.99, 0.02, 3.5, -0.02, 1.01, -1.25])
    # the [6] path as it was before polynomial maps (align.compose_fit's own arithmetic, restated)
    a, t = np.array([[m[0], m[1]], [m[3], m[4]]]), np.array([m[2], m[5]])
    f, c = fit['fit_matrix'], fit['center']
    g = f @ (np.ones(2) - c) + c + fit['offset'] - 1.0
    a2, t2 = a @ f, a @ g + t
    want = np.array([a2[0, 0], a2[0, 1], t2[0], a2[1, 0], a2[1, 1], t2[1]])
    got = align.compose_fit(m, fit)
    assert isinstance(got, np.ndarray) and got.tobytes() == want.tobytes()
    assert align.compose_fit(list(m), dict(fit_matrix=f, offset=fit['offset'])).shape == (6,)
    p = pc.radial3()['maps'][0]
    pg = align.compose_fit(p, fit)
    assert isinstance(pg, PolyMap) and pg.degree == 3
    x, y = _points()
    gx, gy = f[0, 0] * x + f[0, 1] * y + g[0], f[1, 0] * x + f[1, 1] * y + g[1]
    assert np.abs(np.array(pg(x, y)) - np.array(p(gx, gy))).max() < 1e-10
    # a degree-1 PolyMap composes to the affine result
    pa = align.compose_fit(PolyMap.from_affine(m, (10.0, 20.0)), fit)
    assert np.allclose(pa.affine(), want, rtol=0, atol=1e-11)


# ---------------------------------------------------------------------------------------------------------------
# DeviceDrizzle, before the device
# ---------------------------------------------------------------------------------------------------------------
def _host_drizzle(maps, K=3, **kw):
    from subpixal_amd import resample
    frames = [np.zeros((40, 48), np.float32) for _ in range(K)]
    a = dict(frames=frames, maps=maps, out_shape=(37, 70), names=['a', 'b', 'c'][:K])
    a.update(kw)
    return resample.DeviceDrizzle(**a)


def test_python_argument_errors_before_the_device():
    from subpixal_amd.resample import PolyMap
    p, a6 = pc.radial3()['maps'][0], [1.0, 0, 0, 0, 1, 0]
    d = _host_drizzle([a6, p, np.array(a6)])
    assert d.map('b') is p and list(d.map('a')) == a6 and d.output_sci is None
    d.map('a')[2] = 9
    assert d.map('a')[2] == 0
    for maps, what in (([a6, p], 'maps'), ([a6, p, [1.0, 0, 0, 2, 0, 0]], 'singular'),
                       ([a6, p, [1.0, 0, np.nan, 0, 1, 0]], 'finite'), ([a6, p, [1.0, 0, 0]], 'maps')):
        with pytest.raises(ValueError, match=what):
            _host_drizzle(maps)
    with pytest.raises(ValueError, match='kernel'):
        _host_drizzle([p, p, p], kernel='gaussian')
    with pytest.raises(ValueError, match='cr_reject'):
        _host_drizzle([a6, p, a6], cr_reject=True, rms=0.1)
    with pytest.raises(ValueError, match='cr_reject'):
        d.set_config_parameters(cr_reject=True, rms=0.1)
    assert not d._cr['on']
    e = _host_drizzle([a6, a6, a6], cr_reject=True, rms=0.1)
    with pytest.raises(ValueError, match='cr_reject'):
        e.set_map('b', p)
    assert list(e.map('b')) == a6
    with pytest.raises(ValueError, match='singular'):
        d.set_map('b', [0, 0, 0, 0, 0, 0])
    with pytest.raises(ValueError, match='no frame'):
        d.set_map('z', p)
    assert d.map('b') is p
    q = d.copy()
    q.set_map('a', PolyMap.from_affine(a6))
    assert isinstance(q.map('a'), PolyMap) and list(d.map('a')) == a6 and q._pool['a'] is d._pool['a']


def test_shifted_poly_maps_are_the_map_about_each_cutout_centre_and_inverse_holds_at_large_coordinates():
    """`align.shifted_poly_maps` (all sources at once) against `PolyMap.about` source by source; the Newton inverse on
    a 4096 px frame, where 1e-12 px is below what float64 resolves"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import bench_drizzle_poly as bp
    from subpixal_amd import align
    from subpixal_amd.resample import PolyMap
    m = bp.distortion(4096, 3, 0.37, -0.21)
    r = np.random.RandomState(4)
    centers = np.round(r.uniform(20, 4070, (50, 2)) * 2) / 2
    origins = np.round(r.uniform(0, 4000, (50, 2)))
    coef = align.shifted_poly_maps(m, centers, origins)
    assert coef.shape == (50, 2, 21)
    for n in (0, 17, 49):
        want = m.about(centers[n]).coef.copy()
        want[:, 0] -= origins[n]
        assert np.abs(coef[n] - want).max() <= 1e-12 * 4096
        p = PolyMap(coef[n], 3, centers[n])
        x, y = centers[n] + r.uniform(-30, 30, (2, 20, 1))
        assert np.abs(np.array(p(x, y)) + origins[n][:, None, None] - np.array(m(x, y))).max() < 1e-9
    x, y = r.uniform(0, 4095, (2, 1000))
    xi, yi = m.inverse(*m(x, y))
    assert max(np.abs(xi - x).max(), np.abs(yi - y).max()) <= 1e-10
