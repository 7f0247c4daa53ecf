"""Source finding without a GPU: the kernels of subpixal_amd/csrc/spx_detect_kernels.h on CPU threads
(tests/cpu_emu/emu_detect.cpp, launched as spx_capi.hip launches them) against the numpy/scipy statement of
tests/detect_statement.py; the new C entries' argument checks; `detect.find_sources`' argument errors.

The CPU harness runs workgroups one after another with real threads inside: it proves logic, index arithmetic
and the LDS union-find under true concurrency, not the races between workgroups (tests/test_gpu_detect.py).
Frame sides are not multiples of the 64 x 32 tile.  SPX_EMU_DETECT_LIB: a pre-built (sanitizer) harness."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import detect_statement as ds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'subpixal_amd', 'csrc')
NEW = ('spx_detect_workspace_bytes', 'spx_detect_label_f32', 'spx_detect_label_f64', 'spx_measure_labels_f32',
       'spx_measure_labels_f64')
E_ARG, E_SHAPE, E_WORKSPACE = -1, -2, -4
_LIB = {}


@pytest.fixture(scope='module')
def emud(tmp_path_factory):
    if 'lib' not in _LIB:
        so = os.environ.get('SPX_EMU_DETECT_LIB')
        if not so:
            out = subprocess.check_output(['make', '-s', '-C', CSRC, '--eval',
                                           'spx-emu-flags: ; @echo $(HOSTCXX) $(EMUFLAGS)', 'spx-emu-flags'],
                                          universal_newlines=True).split()
            so = str(tmp_path_factory.mktemp('emud') / 'libspx_emu_detect.so')
            subprocess.check_call(out + ['-shared', '-o', so, os.path.join(ROOT, 'tests', 'cpu_emu', 'emu_detect.cpp')])
        _LIB['lib'] = ctypes.CDLL(so)
    return _LIB['lib']


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def run_emu(lib, frame, thr, bkg=0.0, mask=None, filt=None, min_area=1, conn=8, grid=3):
    """the pipeline of detect.find_sources on the harness: (labels, table, flags, bbox)"""
    f64 = frame.dtype == np.float64
    frame = np.ascontiguousarray(frame)
    ny, nx = frame.shape
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    thr_map = np.ascontiguousarray(thr, np.float32) if np.ndim(thr) else None
    k = None if filt is None else np.ascontiguousarray(filt, frame.dtype)
    fky, fkx = (1, 1) if k is None else k.shape
    labels = np.full((ny, nx), -5, np.int32)
    nlab = np.full(1, -5, np.int32)
    sc = (ctypes.c_double if f64 else ctypes.c_float)(0.0 if thr_map is not None else float(thr))
    fn = lib.emud_detect_label_f64 if f64 else lib.emud_detect_label_f32
    assert fn(_p(frame), _p(m), sc, _p(thr_map), _p(k), fky, fkx, ny, nx, conn, min_area, _p(labels), _p(nlab),
              grid) == 0
    n = int(nlab[0])
    assert n >= 0
    boxes = np.zeros((n + 1, 4), np.int32)
    counts = np.zeros(n + 1, np.int32)
    assert lib.emud_label_bboxes(_p(labels), ny, nx, n, _p(boxes), _p(counts), grid) == 0
    table = np.full((n, len(ds.COLS)), -5.0)
    flags = np.full(n, -5, np.int32)
    bkg_map = np.ascontiguousarray(bkg, frame.dtype) if np.ndim(bkg) else None
    fn = lib.emud_measure_f64 if f64 else lib.emud_measure_f32
    assert fn(_p(frame), _p(m), ctypes.c_double(0.0 if bkg_map is not None else float(bkg)), _p(bkg_map), _p(labels),
              ny, nx, n, _p(boxes), _p(table), _p(flags), grid) == 0
    return labels, table, flags, boxes[1:]


def _check(lib, what, frame, thr, **kw):
    st = ds.statement(frame, thr, **kw)
    got = run_emu(lib, frame, thr, **kw)
    return ds.check(*got, st, what=what), st


# ---------------------------------------------------------------------------------------------------------------
# scenes.  Pixel values are multiples of 2^-10 well away from the thresholds, so no value is within rounding of
# one (detect_statement.statement asserts it) and float32 holds them exactly.
# ---------------------------------------------------------------------------------------------------------------
def _values(rng, shape, lo=2.0, hi=6.0):
    return np.round(rng.uniform(lo, hi, shape) * 1024) / 1024


def spiral(ny, nx, rng, dtype):
    """one 1-pixel-wide rectangular spiral over the whole frame (arms 2 px apart): a single component with a
    union chain through every tile"""
    on = np.zeros((ny, nx), bool)
    y0, x0, y1, x1 = 0, 0, ny - 1, nx - 1
    y, x = 0, 0
    on[0, 0] = True
    while x1 - x0 >= 2 and y1 - y0 >= 2:
        on[y0, x0:x1 + 1] = True
        on[y0:y1 + 1, x1] = True
        on[y1, x0 + 2:x1 + 1] = True
        on[y0 + 2:y1 + 1, x0 + 2] = True
        y0, x0, y1, x1 = y0 + 2, x0 + 2, y1 - 2, x1 - 2
        on[y0, x0] = True
    return np.where(on, _values(rng, on.shape), 0.0).astype(dtype)


def comb(ny, nx, rng, dtype):
    """teeth every other column hanging from a spine along the LAST row: every tooth is its own component
    until the bottom tile row joins them, and the root (first pixel) sits in the first tile"""
    on = np.zeros((ny, nx), bool)
    on[:, ::2] = True
    on[-1, :] = True
    return np.where(on, _values(rng, on.shape), 0.0).astype(dtype)


def dominoes(ny, nx, rng, dtype):
    """a checkerboard of 2 x 1 cells: 4-connectivity sees every cell on its own, 8-connectivity one component
    (2 x 1 rather than 1 x 1 cells so that every source has a direction: theta is defined)"""
    yy, xx = np.mgrid[0:ny, 0:nx]
    on = ((xx // 2) + yy) % 2 == 0
    return np.where(on, _values(rng, on.shape), 0.0).astype(dtype)


def blobs(ny, nx, rng, dtype, nblob=40):
    """elongated Gaussian blobs on zero background"""
    yy, xx = np.mgrid[0:ny, 0:nx]
    f = np.zeros((ny, nx))
    for _ in range(nblob):
        cy, cx = rng.uniform(0, ny), rng.uniform(0, nx)
        sy, sx = rng.uniform(0.8, 1.6), rng.uniform(1.8, 3.0)
        th = rng.uniform(0, np.pi)
        u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th)
        v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
        f += rng.uniform(3, 9) * np.exp(-0.5 * ((u / sx) ** 2 + (v / sy) ** 2))
    return f.astype(dtype)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_spiral_and_comb_one_label_through_every_tile(emud, dtype):
    rng = np.random.default_rng(3)
    for name, f in (('spiral', spiral(75, 139, rng, dtype)), ('comb', comb(70, 131, rng, dtype))):
        for conn in (8, 4):
            res, st = _check(emud, '%s conn %d %s' % (name, conn, np.dtype(dtype)), f, 1.0, conn=conn)
            assert st['n'] == 1
            assert st['flags'][0] & 1                   # touches the border


def test_domino_checkerboard_4_against_8(emud):
    f = dominoes(37, 70, np.random.default_rng(4), np.float32)
    res8, st8 = _check(emud, 'dominoes conn 8', f, 1.0, conn=8)
    res4, st4 = _check(emud, 'dominoes conn 4', f, 1.0, conn=4)
    assert st8['n'] == 1 and st4['n'] > 600


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_full_and_empty_frames(emud, dtype):
    f = _values(np.random.default_rng(5), (41, 77)).astype(dtype)
    res, st = _check(emud, 'full', f, 1.0)
    assert st['n'] == 1 and st['table']['npix'][0] == f.size and st['flags'][0] == 1
    res, st = _check(emud, 'empty', f, 100.0)
    assert st['n'] == 0
    res, st = _check(emud, 'one row', f[:1], 1.0)          # a frame lower than a tile, and a 1 x 2 frame
    res, st = _check(emud, 'two pixels', f[:1, :2], 1.0, min_area=1)
    assert st['n'] == 1


def test_min_area_removes_first_middle_and_last(emud):
    f = np.zeros((70, 150), np.float32)
    rng = np.random.default_rng(6)
    # small components (2..3 px: a single pixel has no direction) at the start, in the middle and at the end of the numbering, big ones between
    f[0, 0:2] = 3.0
    f[0, 5:7] = 3.5
    for cy, cx in ((10, 20), (30, 62), (33, 100), (50, 30), (60, 120)):
        f[cy - 3:cy + 4, cx - 5:cx + 6] = _values(rng, (7, 11))
    f[20, 62:65] = 2.5                                       # 3 px, between the big ones, across a tile border
    f[40:42, 3] = 4.0
    f[69, 148:150] = 2.25
    f[69, 140:142] = 2.0
    for min_area in (1, 3, 4, 77, 78):
        res, st = _check(emud, 'min_area %d' % min_area, f, 1.0, min_area=min_area)
    assert ds.statement(f, 1.0, min_area=4)['n'] == 5 and ds.statement(f, 1.0, min_area=1)['n'] == 11
    assert ds.statement(f, 1.0, min_area=3)['n'] == 6
    assert ds.statement(f, 1.0, min_area=78)['n'] == 0


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_blobs_mask_nonfinite_threshold_map_background(emud, dtype):
    rng = np.random.default_rng(7)
    f = blobs(83, 157, rng, dtype)
    f += np.asarray(1.0 / 2048, dtype)                       # keeps every value off the thresholds below
    mask = rng.random(f.shape) < 0.01
    f[rng.random(f.shape) < 0.005] = np.nan
    f[rng.random(f.shape) < 0.003] = np.inf
    f[rng.random(f.shape) < 0.002] = -np.inf
    thr_map = (0.5 + 0.25 * (np.arange(f.shape[1]) // 16 % 2))[None, :] * np.ones(f.shape, np.float32)
    bkg_map = np.full(f.shape, 1.0 / 64, dtype)
    _check(emud, 'blobs scalar', f, 0.75, mask=mask, min_area=3)
    _check(emud, 'blobs thr map', f, thr_map.astype(np.float32), mask=mask, min_area=3, conn=4)
    _check(emud, 'blobs bkg map', f, 0.75, bkg=bkg_map, mask=mask, min_area=3)
    # a background above the pixels: flux <= 0 -> flag bit 1, positions NaN
    res, st = _check(emud, 'blobs high background', f, 0.75, bkg=50.0, min_area=3)
    assert np.all(st['flags'] & 2)
    # one bad pixel inside the box of a source but outside the source: flag bit 2
    g = np.zeros((40, 70), dtype)
    g[10:15, 10:20] = 2.0
    g[12, 14] = np.nan
    res, st = _check(emud, 'hole', g, 1.0)
    assert st['n'] == 1 and st['flags'][0] == 4 and st['table']['npix'][0] == 49


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_filters_3x3_and_7x5(emud, dtype):
    rng = np.random.default_rng(8)
    f = blobs(71, 133, rng, dtype, nblob=30)
    f[rng.random(f.shape) < 0.004] = np.nan
    mask = rng.random(f.shape) < 0.01
    k3 = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]]) / 16.0
    k75 = np.round(np.outer(np.exp(-0.5 * (np.arange(-3, 4) / 1.5) ** 2),
                            np.exp(-0.5 * (np.arange(-2, 3) / 1.0) ** 2)) * 64) / 512.0
    k75[0, 0] = -1.0 / 512                                   # not symmetric: a convolution would differ
    assert k75.shape == (7, 5)
    for name, k, thr in (('3x3', k3, 0.7001), ('7x5', k75, 0.9001)):
        assert not np.array_equal(ds.detection(f, thr, mask, k)[0], ds.detection(f, thr, mask, k[::-1, ::-1])[0]) \
            or name == '3x3'
        _check(emud, 'filter %s' % name, f, thr, mask=mask, filt=k.astype(dtype), min_area=2)
        _check(emud, 'filter %s conn 4' % name, f, thr, filt=k.astype(dtype), min_area=1, conn=4, bkg=0.01)


def test_grid_size_does_not_matter(emud):
    f = blobs(83, 157, np.random.default_rng(9), np.float32)
    a = run_emu(emud, f, 0.7503, min_area=2, grid=1)
    b = run_emu(emud, f, 0.7503, min_area=2, grid=64)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


# ---------------------------------------------------------------------------------------------------------------
# the boundary
# ---------------------------------------------------------------------------------------------------------------
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


def test_c_argument_errors_before_any_hip_call():
    from subpixal_amd import _ffi
    lib = _ffi.load()
    buf = np.zeros(1024, np.float64)
    b = buf.ctypes.data
    need = lib.spx_detect_workspace_bytes(8, 8)
    assert need >= 2 * 4 * 64 + 4 + 4
    assert lib.spx_detect_workspace_bytes(0, 8) == 0 and lib.spx_detect_workspace_bytes(65536, 32768) == 0
    for fn in (lib.spx_detect_label_f32, lib.spx_detect_label_f64):
        def call(frame=b, filt=None, fky=1, fkx=1, fny=8, fnx=8, conn=8, min_area=1, work=b, wb=need, out=b, nl=b):
            return fn(frame, None, 1.0, None, filt, fky, fkx, fny, fnx, conn, min_area, work, wb, out, nl, None)
        assert call(frame=None) == E_ARG and call(out=None) == E_ARG and call(nl=None) == E_ARG
        assert call(conn=6) == E_ARG and call(conn=0) == E_ARG
        assert call(min_area=0) == E_ARG
        assert call(filt=b, fky=2, fkx=3) == E_ARG and call(filt=b, fky=3, fkx=4) == E_ARG
        assert call(filt=b, fky=9, fkx=3) == E_ARG and call(filt=b, fky=3, fkx=9) == E_ARG
        assert call(fny=0) == E_SHAPE and call(fny=65536, fnx=32768) == E_SHAPE
        assert call(work=None) == E_WORKSPACE and call(wb=need - 1) == E_WORKSPACE
    for fn in (lib.spx_measure_labels_f32, lib.spx_measure_labels_f64):
        assert fn(b, None, 0.0, None, b, 8, 8, -1, b, b, b, None) == E_ARG
        assert fn(None, None, 0.0, None, b, 8, 8, 1, b, b, b, None) == E_ARG
        assert fn(b, None, 0.0, None, b, 0, 8, 1, b, b, b, None) == E_SHAPE
        assert fn(None, None, 0.0, None, None, 8, 8, 0, None, None, None, None) == 0       # nothing to measure


def test_find_sources_argument_errors():
    from subpixal_amd import detect
    f = np.zeros((8, 9), np.float32)
    with pytest.raises(ValueError, match='connectivity'):
        detect.find_sources(f, 1.0, connectivity=6)
    with pytest.raises(ValueError, match='min_area'):
        detect.find_sources(f, 1.0, min_area=0)
    with pytest.raises(ValueError, match='odd'):
        detect.find_sources(f, 1.0, filter_kernel=np.ones((2, 3)))
    with pytest.raises(ValueError, match='at most 7'):
        detect.find_sources(f, 1.0, filter_kernel=np.ones((3, 9)))
    with pytest.raises(ValueError, match='mask'):
        detect.find_sources(f, 1.0, mask=np.zeros((8, 8), bool))
    with pytest.raises(ValueError, match='2-D'):
        detect.find_sources(np.zeros(8, np.float32), 1.0)
    import subpixal_amd
    assert subpixal_amd.detect is detect
