"""The error measurements without a GPU: the kernel of subpixal_amd/csrc/spx_error_kernels.h on CPU threads
(tests/cpu_emu/emu_errors.cpp, launched as spx_capi.hip launches it) against the numpy statement of
tests/errors_statement.py -- nhalf, fwhm (to the bit), the flags and the NaN pattern exactly, the four sums within
the derived bounds; the new C entries' argument checks; the ValueErrors of `detect.measure_errors`,
`detect.find_sources`, `detect.detect_sources` and `Sources.cutout_catalog`.

The measure table both sides read (flux, x, y, peak) is the emulated measure kernel's output for the scene.
SPX_EMU_ERRORS_LIB: a pre-built harness."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import errors_cases as ec
import errors_statement as es

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'subpixal_amd', 'csrc')
NEW = ('spx_measure_errors_f32', 'spx_measure_errors_f64')
E_ARG, E_SHAPE = -1, -2
DTYPES = (np.float32, np.float64)
_LIB = {}
_vp, _int, _dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double


@pytest.fixture(scope='module')
def emue(tmp_path_factory):
    if 'lib' not in _LIB:
        so = os.environ.get('SPX_EMU_ERRORS_LIB')
        if not so:
            out = subprocess.check_output(['make', '-s', '-C', CSRC, '--eval',
                                           'spx-emu-flags: ; @echo $(HOSTCXX) $(EMUFLAGS)', 'spx-emu-flags'],
                                          universal_newlines=True).split()
            so = str(tmp_path_factory.mktemp('emue') / 'libspx_emu_errors.so')
            subprocess.check_call(out + ['-shared', '-o', so, os.path.join(ROOT, 'tests', 'cpu_emu', 'emu_errors.cpp')])
        lib = ctypes.CDLL(so)
        for fn in (lib.emud_measure_f32, lib.emud_measure_f64):
            fn.argtypes = [_vp, _vp, _dbl, _vp, _vp, _int, _int, _int, _vp, _vp, _vp, _int]
        for fn in (lib.emue_errors_f32, lib.emue_errors_f64):
            fn.argtypes = [_vp, _vp, _dbl, _vp, _dbl, _vp, _dbl, _vp, _int, _int, _int, _vp, _vp, _vp, _vp, _int]
        lib.emud_label_bboxes.argtypes = [_vp, _int, _int, _int, _vp, _vp, _int]
        _LIB['lib'] = lib
    return _LIB['lib']


def _p(a):
    return None if a is None else a.ctypes.data_as(_vp)


def _split(v, dtype):
    """(scalar, map or None) the way the C entries take a background or an rms"""
    if np.ndim(v):
        return 0.0, np.ascontiguousarray(v, dtype)
    return float(v), None


def prepare(lib, s, dtype):
    """the scene in `dtype` with boxes and the measure table from the emulated kernels"""
    frame = np.ascontiguousarray(s['frame'], dtype)
    ny, nx = frame.shape
    n = s['n']
    labels = s['labels']
    m = None if s['mask'] is None else np.ascontiguousarray(s['mask'], np.uint8)
    bkg, bkg_map = _split(s['bkg'], dtype)
    rms, rms_map = _split(s['rms'], dtype)
    boxes = np.full((n + 1, 4), -9, np.int32)
    counts = np.full(n + 1, -9, np.int32)
    assert lib.emud_label_bboxes(_p(labels), ny, nx, n, _p(boxes), _p(counts), 3) == 0
    assert np.array_equal(boxes, es.bboxes(labels, n))
    table = np.full((n, 13), -9.0)
    flags = np.full(n, -9, np.int32)
    fn = lib.emud_measure_f64 if dtype == np.float64 else lib.emud_measure_f32
    assert fn(_p(frame), _p(m), bkg, _p(bkg_map), _p(labels), ny, nx, n, _p(boxes), _p(table), _p(flags), 3) == 0
    return dict(frame=frame, labels=labels, n=n, m=m, bkg=bkg, bkg_map=bkg_map, rms=rms, rms_map=rms_map, boxes=boxes,
                table=table, mflags=flags, gain=s['gain'], mask=s['mask'])


def run_emu(lib, a, grid=3, **over):
    a = dict(a, **over)
    n = a['n']
    ny, nx = a['frame'].shape
    out = np.full((n, 6), -9.0)
    eflags = np.full(n, -9, np.int32)
    fn = lib.emue_errors_f64 if a['frame'].dtype == np.float64 else lib.emue_errors_f32
    assert fn(_p(a['frame']), _p(a['m']), a['bkg'], _p(a['bkg_map']), a['rms'], _p(a['rms_map']),
              0.0 if a['gain'] is None else a['gain'], _p(a['labels']), ny, nx, n, _p(a['boxes']), _p(a['table']),
              _p(out), _p(eflags), grid) == 0
    return out, eflags


def state(a):
    return es.statement(a['frame'], a['labels'], a['n'], a['table'],
                        a['rms_map'] if a['rms_map'] is not None else a['rms'],
                        bkg=a['bkg_map'] if a['bkg_map'] is not None else a['bkg'], gain=a['gain'], mask=a['mask'])


def both(lib, name, dtype, **over):
    a = dict(prepare(lib, ec.ALL[name](), dtype), **over)
    st = state(a)
    out, eflags = run_emu(lib, a)
    es.check(out, eflags, st, what='%s %s' % (name, np.dtype(dtype).name))
    return a, st, out, eflags


# ---------------------------------------------------------------------------------------------------------------
# the scenes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', sorted(ec.ALL))
def test_scene_against_the_statement(emue, name, dtype):
    both(emue, name, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
def test_one_pixel_segment(emue, dtype):
    a, st, out, eflags = both(emue, 'one_pixel', dtype)
    # x = 4, y = 3 exactly: u = 0, no position variance; the one pixel is its own half maximum
    assert out[0, 0] == np.sqrt(0.05 * 0.05)                 # (a scalar rms is a double, whatever the frame's dtype)
    assert list(out[0, 1:5]) == [0.0, 0.0, 0.0, 1.0] and out[0, 5] == 2.0 * np.sqrt(1.0 / np.pi)
    assert eflags[0] == es.FLAG_HALFMAX


@pytest.mark.parametrize('dtype', DTYPES)
def test_boxes_beyond_one_pass_of_the_workgroup(emue, dtype):
    a, st, out, eflags = both(emue, 'big_boxes', dtype)
    area = (a['boxes'][1:, 2] - a['boxes'][1:, 0] + 1) * (a['boxes'][1:, 3] - a['boxes'][1:, 1] + 1)
    assert area.min() > 256 and area.max() > 2048 and list(eflags) == [0, 0]
    assert np.all(out[:, 4] < st['npix'])


def test_ring_leaves_the_labels_inside_its_box_alone(emue):
    a, st, out, eflags = both(emue, 'ring', np.float32)
    # the ring alone in the frame gives the ring's row again, bit for bit: the others do not leak into its sums
    s = ec.ring()
    alone = dict(s, labels=np.where(s['labels'] == 1, 1, 0).astype(np.int32), n=1)
    b = prepare(emue, alone, np.float32)
    o1, f1 = run_emu(emue, b)
    assert o1[0].tobytes() == out[0].tobytes() and f1[0] == eflags[0]


@pytest.mark.parametrize('dtype', DTYPES)
def test_masked_and_nan_pixels_are_not_summed(emue, dtype):
    a, st, out, eflags = both(emue, 'bad_pixels', dtype)
    assert st['npix'][0] == (a['labels'] == 1).sum() - 2 and a['mflags'][0] & 4


@pytest.mark.parametrize('dtype', DTYPES)
def test_bad_rms_pixels_count_as_zero_and_raise_the_flag(emue, dtype):
    a, st, out, eflags = both(emue, 'bad_rms', dtype)
    assert list(eflags & es.FLAG_NOISE) == [0, 64, 64, 0]         # a zero is a legal rms: no flag
    # the same scene with those pixels set to 0 outright: the same numbers, no flag
    clean = a['rms_map'].copy()
    clean[~np.isfinite(clean) | (clean < 0)] = 0
    o2, f2 = run_emu(emue, a, rms_map=clean)
    assert o2.tobytes() == out.tobytes() and list(f2 & es.FLAG_NOISE) == [0, 0, 0, 0]


@pytest.mark.parametrize('dtype', DTYPES)
def test_gain_adds_shot_noise_on_positive_pixels_only(emue, dtype):
    off = both(emue, 'negative_w_gain_off', dtype)
    on = both(emue, 'negative_w_gain_on', dtype)
    a = off[0]
    w = a['frame'].astype(np.float64) - a['bkg']
    sel = (a['labels'] == 1)
    assert (w[sel] < 0).sum() > 10
    # fluxerr^2 grows by sum of w / gain over the positive pixels, and by nothing else
    extra = (w[sel & (w > 0)] / 2.0).sum()
    assert abs((on[2][0, 0] ** 2 - off[2][0, 0] ** 2) - extra) <= 1e-12 * extra
    # a gain that is not positive and finite is "off"
    for g in (0.0, -1.0, float('nan'), float('inf')):
        o, f = run_emu(emue, a, gain=g)
        assert o.tobytes() == off[2].tobytes() and f.tobytes() == off[3].tobytes()


@pytest.mark.parametrize('dtype', DTYPES)
def test_segment_without_flux(emue, dtype):
    a, st, out, eflags = both(emue, 'no_flux', dtype)
    assert a['mflags'][0] & 2 and not a['mflags'][1] & 2
    assert np.all(np.isnan(out[0, 1:4])) and out[0, 0] > 0 and out[0, 4] == 0 and np.isnan(out[0, 5])
    assert np.all(np.isfinite(out[1]))


@pytest.mark.parametrize('dtype', DTYPES)
def test_segments_on_the_border(emue, dtype):
    a, st, out, eflags = both(emue, 'border', dtype)
    assert list(a['mflags'] & 1) == [1, 1, 1, 1, 0, 1] and np.all(np.isfinite(out))


def test_plateau_peak_and_flat_segment(emue):
    a, st, out, eflags = both(emue, 'plateau', np.float32)
    assert list(out[:, 4]) == [12.0, 48.0] and list(eflags) == [0, es.FLAG_HALFMAX]
    assert out[1, 5] == 2.0 * np.sqrt(48.0 / np.pi)


@pytest.mark.parametrize('dtype', DTYPES)
def test_no_labels_writes_nothing_and_a_one_pixel_frame(emue, dtype):
    a, st, out, eflags = both(emue, 'empty', dtype)
    assert out.shape == (0, 6)
    a, st, out, eflags = both(emue, 'single_pixel_frame', dtype)
    assert out[0, 0] == np.sqrt(0.25 + 1.5) and eflags[0] == es.FLAG_HALFMAX


@pytest.mark.parametrize('dtype', DTYPES)
def test_grid_size_does_not_matter_and_runs_are_identical(emue, dtype):
    for name in ('bad_rms', 'big_boxes', 'border'):
        a = prepare(emue, ec.ALL[name](), dtype)
        runs = [run_emu(emue, a, grid=g) for g in (1, 3, a['n'] + 5, 3)]
        for o, f in runs[1:]:
            assert o.tobytes() == runs[0][0].tobytes() and f.tobytes() == runs[0][1].tobytes(), name


@pytest.mark.parametrize('dtype', DTYPES)
def test_scalar_rms_equals_a_constant_map(emue, dtype):
    for name in ('ring', 'border', 'no_flux'):
        a = prepare(emue, ec.ALL[name](), dtype)
        c = float(dtype(0.04))                               # the scalar the map's elements hold, widened
        const = np.full(a['frame'].shape, c, dtype)
        o1, f1 = run_emu(emue, a, rms=c, rms_map=None)
        o2, f2 = run_emu(emue, a, rms=0.0, rms_map=const)
        assert o1.tobytes() == o2.tobytes() and f1.tobytes() == f2.tobytes(), name


# ---------------------------------------------------------------------------------------------------------------
# the boundary
# ---------------------------------------------------------------------------------------------------------------
def _declared():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'subpixal_hip.h')).read(), flags=re.S)
    return set(re.findall(r'\b(spx_[a-z0-9_]+)\s*\(', text))


def test_new_entries_exported_and_declared():
    from subpixal_amd import _ffi, detect
    lib = _ffi.load()
    declared = _declared()
    for name in NEW:
        assert name in declared and name in _ffi.EXPORTED_SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    assert declared == set(_ffi.EXPORTED_SYMBOLS)
    assert lib.spx_abi_version() == _ffi.ABI_VERSION == 4
    header = open(os.path.join(ROOT, 'include', 'subpixal_hip.h')).read()
    assert '#define SPX_ERROR_COLUMNS 6' in header and _ffi.ERROR_COLUMNS == 6 == len(detect.ERROR_COLUMNS)
    assert '#define SPX_EFLAG_HALFMAX 32' in header and '#define SPX_EFLAG_NOISE 64' in header
    assert detect.FLAG_HALFMAX == es.FLAG_HALFMAX == 32 and detect.FLAG_NOISE == es.FLAG_NOISE == 64
    assert detect.ERROR_COLUMNS == es.COLS
    table = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in ('spx_measure_errors_f32', '_f64'):
        assert '`%s`' % name in table, name


def test_c_argument_errors_before_any_hip_call():
    from subpixal_amd import _ffi
    lib = _ffi.load()
    buf = np.zeros(1024, np.float64)
    b = buf.ctypes.data
    for fn in (lib.spx_measure_errors_f32, lib.spx_measure_errors_f64):
        def call(frame=b, labels=b, fny=8, fnx=8, nlabels=3, boxes=b, table=b, out=b, eflags=b):
            return fn(frame, None, 0.0, None, 1.0, None, 0.0, labels, fny, fnx, nlabels, boxes, table, out, eflags, None)
        for name in ('frame', 'labels', 'boxes', 'table', 'out', 'eflags'):
            assert call(**{name: None}) == E_ARG, name
            assert b'null' in lib.spx_last_error()
        assert call(nlabels=-1) == E_ARG
        assert call(fny=0) == E_SHAPE and call(fnx=0) == E_SHAPE and call(fny=65536, fnx=32768) == E_SHAPE
        # no labels: success before any pointer is looked at, nothing written
        assert call(nlabels=0) == 0 and call(nlabels=0, frame=None, out=None, table=None) == 0
        assert not buf.any()


def test_python_argument_errors_before_the_device():
    from subpixal_amd import detect
    f = np.zeros((8, 9), np.float32)
    lab = np.zeros((8, 9), np.int32)
    tab = np.zeros((0, 13))
    for kw, what in ((dict(rms=None), 'rms'), (dict(rms=np.zeros((8, 8))), 'rms'), (dict(gain=0.0), 'gain'),
                     (dict(gain=-2.0), 'gain'), (dict(gain=float('nan')), 'gain'), (dict(gain=float('inf')), 'gain'),
                     (dict(mask=np.zeros((8, 8), bool)), 'mask'), (dict(table=np.zeros((2, 13))), 'table'),
                     (dict(table=np.zeros((0, 6))), 'table'), (dict(nlabels=-1), 'nlabels'),
                     (dict(labels=np.zeros((8, 8), np.int32)), 'labels')):
        a = dict(frame=f, labels=lab, nlabels=0, table=tab, rms=0.1)
        a.update(kw)
        with pytest.raises(ValueError, match=what):
            detect.measure_errors(**a)
    for kw, what in ((dict(rms=np.zeros((8, 8))), 'rms'), (dict(rms=0.1, gain=0.0), 'gain'), (dict(gain=2.0), 'rms')):
        with pytest.raises(ValueError, match=what):
            detect.find_sources(f, 1.0, **kw)
    for kw, what in ((dict(errors=True, gain=-1.0), 'gain'), (dict(gain=2.0), 'errors')):
        with pytest.raises(ValueError, match=what):
            detect.detect_sources(f, **kw)
    with pytest.raises(TypeError, match='rms'):
        detect.detect_sources(f, rms=0.1)


class _FakeTensor(object):
    """stands in for the CUDA tensors a Sources holds: only .cpu().numpy() is asked of them here"""
    def __init__(self, a):
        self.a = a

    def cpu(self):
        return self

    def numpy(self):
        return self.a


def _sources(errors):
    from subpixal_amd import detect
    table = np.zeros((3, 13))
    table[:, 1] = [10.0, 20.0, -1.0]
    err = None
    if errors:
        err = np.zeros((3, 6))
        err[:, 0] = [1.0, 4.0, 1.0]                          # fluxerr
        err[:, 4] = [4.0, 9.0, 0.0]                          # nhalf
        err[:, 5] = [2.0, 3.0, np.nan]                       # fwhm
        err = _FakeTensor(err)
    return detect.Sources(None, _FakeTensor(table), _FakeTensor(np.array([0, 0, 2], np.int32)),
                          _FakeTensor(np.zeros((3, 4), np.int32)), errors=err)


def test_sources_columns_with_and_without_errors():
    from subpixal_amd import detect
    plain, full = _sources(False), _sources(True)
    new = detect.ERROR_COLUMNS + ('snr', 'pos_std', 'weight')
    assert not plain.has_errors and not any(hasattr(plain, c) for c in new + ('errors_device',))
    assert not any(c in plain.table() for c in new)
    assert full.has_errors and all(c in full.table() for c in new)
    k = 2.0 * np.sqrt(2.0 * np.log(2.0))
    assert np.array_equal(full.snr[:2], [10.0, 5.0])
    assert np.array_equal(full.pos_std[:2], [2.0 / (k * 10.0 / 1.0), 3.0 / (k * 20.0 / 4.0)])
    assert np.array_equal(full.weight[:2], 1.0 / full.pos_std[:2] ** 2) and np.isnan(full.weight[2])
    assert full.nhalf.dtype == np.int32 and list(full.nhalf) == [4, 9, 0]
    with pytest.raises(ValueError, match='pos_std'):
        plain.cutout_catalog(None, weight='pos_std')
    with pytest.raises(ValueError, match='weight'):
        full.cutout_catalog(None, weight='snr')
