"""Background estimation without a GPU: the kernels of subpixal_amd/csrc/spx_background_kernels.h on CPU threads
(tests/cpu_emu/emu_background.cpp, launched as spx_capi.hip launches them) against the numpy/scipy statement of
tests/background_statement.py; the new C entries' argument checks; `detect.estimate_background`'s argument
errors; the end-to-end scene's own figures.  The cases are those of tests/test_gpu_background.py
(tests/background_cases.py).  The harness also hands out each cell's clipping range, median, mean and std, which
the device entries do not: ranges must be equal and medians bit-equal."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import background_cases as bc
import background_statement as bs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'subpixal_amd', 'csrc')
NEW = ('spx_background_workspace_bytes', 'spx_background_mesh_f32', 'spx_background_mesh_f64',
       'spx_background_maps_f32', 'spx_background_maps_f64')
E_ARG, E_SHAPE, E_WORKSPACE = -1, -2, -4
_LIB = {}


@pytest.fixture(scope='module')
def emub(tmp_path_factory):
    if 'lib' not in _LIB:
        so = os.environ.get('SPX_EMU_BACKGROUND_LIB')
        if not so:
            out = subprocess.check_output(['make', '-s', '-C', CSRC, '--eval',
                                           'spx-emu-flags: ; @echo $(HOSTCXX) $(EMUFLAGS)', 'spx-emu-flags'],
                                          universal_newlines=True).split()
            so = str(tmp_path_factory.mktemp('emub') / 'libspx_emu_background.so')
            subprocess.check_call(out + ['-shared', '-o', so,
                                         os.path.join(ROOT, 'tests', 'cpu_emu', 'emu_background.cpp')])
        _LIB['lib'] = ctypes.CDLL(so)
        _LIB['lib'].emub_cell_lds_bytes.restype = ctypes.c_size_t
    return _LIB['lib']


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def make_run(lib, grid=3):
    def run(frame, box, filter_size=3, mask=None, exclude=None, sigma=3.0, max_iters=10, min_good_fraction=0.5,
            nsigma=2.5, want=(True, True, True)):
        f64 = frame.dtype == np.float64
        frame = np.ascontiguousarray(frame)
        ny, nx = frame.shape
        bh, bw = box
        ncy, ncx = -(-ny // bh), -(-nx // bw)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        lab = None if exclude is None else np.ascontiguousarray(exclude, np.int32)
        mb, mr = np.full((ncy, ncx), -5.0), np.full((ncy, ncx), -5.0)
        ng = np.full((ncy, ncx), -5, np.int32)
        trace = np.full((ncy, ncx, 5), -5.0)
        fn = lib.emub_mesh_f64 if f64 else lib.emub_mesh_f32
        assert fn(_p(frame), _p(m), _p(lab), ny, nx, bh, bw, ctypes.c_double(sigma), max_iters,
                  ctypes.c_double(min_good_fraction), _p(mb), _p(mr), _p(ng), _p(trace), grid) == 0
        planes = np.full((2, 6, ncy, ncx), -5.0)
        bkg = np.full((ny, nx), -5, frame.dtype) if want[0] else None
        rms = np.full((ny, nx), -5, frame.dtype) if want[1] else None
        thr = np.full((ny, nx), -5, np.float32) if want[2] else None
        status = np.full(1, -5, np.int32)
        fn = lib.emub_maps_f64 if f64 else lib.emub_maps_f32
        assert fn(_p(mb), _p(mr), _p(ng), ncy, ncx, bh, bw, filter_size, ny, nx, ctypes.c_double(nsigma), _p(planes),
                  _p(bkg), _p(rms), _p(thr), _p(status), grid) == 0
        if status[0] & 1:
            raise bs.NoGoodCell()
        return dict(mesh_bkg=mb, mesh_rms=mr, ngood=ng, trace=trace, filt_bkg=planes[0, 0], filt_rms=planes[1, 0],
                    bkg=bkg, rms=rms, thr=thr)
    return run


@pytest.mark.parametrize('name,shape,box,dtype', bc.GEOMETRY)
def test_mesh_geometry(emub, name, shape, box, dtype):
    f = bc.sky(shape, 3, dtype)
    st, got = bc.check_case(make_run(emub), f, box, '%s %s' % (name, np.dtype(dtype)), expect_trace=True)
    ncy, ncx = st['filt_bkg'].shape
    assert (ncy, ncx) == (-(-shape[0] // box[0]), -(-shape[1] // box[1]))
    if name == 'one cell':
        assert np.all(got['bkg'] == got['bkg'][0, 0]) and np.all(got['rms'] == got['rms'][0, 0])
    if name == 'one knot in y':
        assert np.array_equal(got['bkg'], np.repeat(got['bkg'][:1], shape[0], axis=0))
    if name == 'two knots':                  # linear between the knots: second differences vanish to rounding
        inner = got['bkg'].astype(np.float64)[32:95, 32:95]
        assert np.abs(np.diff(inner, 2, axis=0)).max() <= 8 * np.finfo(dtype).eps * np.abs(inner).max()
    if name == 'largest cells':
        assert emub.emub_cell_lds_bytes(np.dtype(dtype).itemsize, *box) == 272 * 8 + 65536


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_blob_clips_in_several_rounds_and_takes_the_median(emub, dtype):
    st, got = bc.check_case(make_run(emub), bc.blob_scene(dtype), (32, 32), 'blob %s' % np.dtype(dtype),
                            expect_trace=True)
    bc.check_blob_cell(st, got)
    # no clipping: the same cell is far off; 40 rounds: the clip converges (the range stops changing) before they are up
    st0, got0 = bc.check_case(make_run(emub), bc.blob_scene(dtype), (32, 32), 'blob, max_iters=0', expect_trace=True,
                              max_iters=0)
    assert st0['mesh']['cells'][(1, 1)]['rounds'] == 0 and got0['mesh_rms'][1, 1] > 5 * got['mesh_rms'][1, 1]
    st40, got40 = bc.check_case(make_run(emub), bc.blob_scene(dtype), (32, 32), 'blob, max_iters=40',
                                expect_trace=True, max_iters=40)
    assert 10 < st40['mesh']['cells'][(1, 1)]['rounds'] < 40


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_constant_frame(emub, dtype):
    f = np.full((50, 70), 3.25, dtype)
    st, got = bc.check_case(make_run(emub), f, (16, 24), 'constant', expect_trace=True)
    assert np.all(got['bkg'] == 3.25) and np.all(got['rms'] == 0) and np.all(got['thr'] == 3.25)
    assert np.all(got['mesh_rms'] == 0)


@pytest.mark.parametrize('fs', [1, 3, 5])
def test_filter_sizes(emub, fs):
    f = bc.with_blob(bc.sky((150, 203), 6, np.float32), 70.0, 100.0, amp=80.0, sig=20.0)
    st, got = bc.check_case(make_run(emub), f, (32, 48), 'filter %d' % fs, filter_size=fs)
    if fs == 1:
        assert np.array_equal(got['filt_bkg'], got['mesh_bkg'])
    else:
        assert not np.array_equal(got['filt_bkg'], got['mesh_bkg'])


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_bad_pixels_mask_and_exclude(emub, dtype):
    rng = np.random.default_rng(7)
    f = bc.sky((100, 130), 8, dtype)
    f[rng.random(f.shape) < 0.01] = np.nan
    f[rng.random(f.shape) < 0.005] = np.inf
    f[rng.random(f.shape) < 0.005] = -np.inf
    mask = rng.random(f.shape) < 0.05
    mask[32:64, 48:96] = True                                  # one cell fully masked: filled from its window
    st, got = bc.check_case(make_run(emub), f, (32, 48), 'bad data', mask=mask, expect_trace=True)
    assert st['mesh']['ngood'][1, 1] == 0 and not st['mesh']['good'][1, 1] and np.isfinite(got['filt_bkg'][1, 1])
    labels = np.zeros(f.shape, np.int32)
    labels[10:30, 10:40] = 3
    labels[70:75, 100:130] = 9
    g = bc.with_blob(f, 20.0, 25.0, amp=500.0, sig=5.0)
    st2, got2 = bc.check_case(make_run(emub), g, (32, 48), 'exclude', mask=mask, exclude=labels)
    st3 = bs.statement(g, (32, 48), mask=mask)
    assert st2['mesh']['ngood'][0, 0] < st3['mesh']['ngood'][0, 0]
    assert abs(st2['mesh']['bkg'][0, 0] - 100.5) < abs(st3['mesh']['bkg'][0, 0] - 100.5) + 0.5


def test_isolated_good_cell_and_no_good_cell(emub):
    f = bc.sky((64, 80), 9, np.float32)
    mask = np.ones(f.shape, bool)
    mask[0:16, 0:16] = False
    st, got = bc.check_case(make_run(emub), f, (16, 16), 'isolated good cell', mask=mask)
    assert st['mesh']['good'].sum() == 1
    assert np.all(got['filt_bkg'] == got['mesh_bkg'][0, 0]) and np.all(got['filt_rms'] == got['mesh_rms'][0, 0])
    # two good cells far apart: the cells between take the global median, the mean of the two
    mask[48:64, 64:80] = False
    st, got = bc.check_case(make_run(emub), f, (16, 16), 'two good cells', mask=mask)
    assert got['filt_bkg'][1, 2] == 0.5 * (got['mesh_bkg'][0, 0] + got['mesh_bkg'][3, 4])
    with pytest.raises(bs.NoGoodCell):
        make_run(emub)(f, (16, 16), mask=np.ones(f.shape, bool))
    with pytest.raises(bs.NoGoodCell):
        bs.statement(f, (16, 16), mask=np.ones(f.shape, bool))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_rms_is_clamped_at_zero(emub, dtype):
    f = bc.undershoot_scene(dtype)
    st, got = bc.check_case(make_run(emub), f, (8, 8), 'undershoot', filter_size=1)
    assert bs.expand(st['filt_rms'], f.shape, (8, 8)).min() < -1e-3          # the spline does dip below zero
    assert got['rms'].min() == 0.0


def test_null_outputs_grid_size_and_repeat(emub):
    f = bc.sky((70, 90), 10, np.float32)
    a = make_run(emub, grid=1)(f, (16, 24))
    b = make_run(emub, grid=64)(f, (16, 24))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    c = make_run(emub)(f, (16, 24), want=(False, False, True))
    assert c['bkg'] is None and c['rms'] is None and c['thr'].tobytes() == a['thr'].tobytes()
    d = make_run(emub)(f, (16, 24), want=(True, False, False))
    assert d['bkg'].tobytes() == a['bkg'].tobytes()


def test_end_to_end_scene_is_within_its_cap_in_the_statement():
    f, true_bkg, sigma = bc.e2e_scene()
    st = bs.statement(f, (64, 64), nsigma=bc.E2E_NSIGMA)
    est = bc.host_sources(f, st['thr'], st['bkg'])
    ref = bc.host_sources(f, true_bkg + bc.E2E_NSIGMA * sigma, true_bkg)
    share = bc.unmatched_share(est, ref)
    print('end-to-end scene: %d sources with the statement, %d with the truth, unmatched share %.4f'
          % (len(est), len(ref), share))
    assert 70 <= len(ref) <= 90
    assert share == bc.E2E_STATEMENT_SHARE <= bc.E2E_UNMATCHED_CAP
    assert not np.any(np.abs(f.astype(np.float64) - st['thr']) <= st['bthr']), 'a pixel within rounding of the threshold'


# ---------------------------------------------------------------------------------------------------------------
# the boundary
# ---------------------------------------------------------------------------------------------------------------
def test_new_entries_exported():
    from subpixal_amd import _ffi
    lib = _ffi.load()
    for name in NEW:
        assert name in _ffi.EXPORTED_SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.spx_abi_version() == _ffi.ABI_VERSION == 4


def test_c_argument_errors_before_any_hip_call():
    from subpixal_amd import _ffi
    lib = _ffi.load()
    buf = np.zeros(4096, np.float64)
    b = buf.ctypes.data
    need = lib.spx_background_workspace_bytes(100, 130, 32, 48)
    assert need >= 2 * 6 * 4 * 3 * 8 + 4
    for bad in ((0, 8, 8, 8), (8, 8, 7, 8), (8, 8, 8, 129), (8, 8, 128, 129), (65536, 32768, 8, 8)):
        assert lib.spx_background_workspace_bytes(*bad) == 0
    for fn, big in ((lib.spx_background_mesh_f32, (128, 128)), (lib.spx_background_mesh_f64, (128, 64))):
        def call(frame=b, fny=100, fnx=130, bh=32, bw=48, kappa=3.0, iters=10, mgf=0.5, o1=b, o2=b, o3=b):
            return fn(frame, None, None, fny, fnx, bh, bw, kappa, iters, mgf, o1, o2, o3, None)
        assert call(frame=None) == E_ARG and call(o1=None) == E_ARG and call(o2=None) == E_ARG and call(o3=None) == E_ARG
        assert call(kappa=0.0) == E_ARG and call(kappa=float('nan')) == E_ARG and call(iters=-1) == E_ARG
        assert call(mgf=-0.1) == E_ARG and call(mgf=1.5) == E_ARG
        assert call(bh=7) == E_SHAPE and call(bw=129) == E_SHAPE and call(fny=0) == E_SHAPE
        assert call(bh=big[0], bw=2 * big[1]) == E_SHAPE
        assert call(fny=65536, fnx=32768) == E_SHAPE
    assert lib.spx_background_mesh_f64(b, None, None, 200, 200, 128, 128, 3.0, 10, 0.5, b, b, b, None) == E_SHAPE
    for fn in (lib.spx_background_maps_f32, lib.spx_background_maps_f64):
        def call(mb=b, ng=b, ncy=4, ncx=3, bh=32, bw=48, fs=3, fny=100, fnx=130, work=b, wb=need, o=(b, b, b), st=b):
            return fn(mb, b, ng, ncy, ncx, bh, bw, fs, fny, fnx, 2.0, work, wb, o[0], o[1], o[2], st, None)
        assert call(mb=None) == E_ARG and call(ng=None) == E_ARG and call(st=None) == E_ARG
        assert call(o=(None, None, None)) == E_ARG
        assert call(fs=2) == E_ARG and call(fs=9) == E_ARG and call(fs=0) == E_ARG
        assert call(bh=4) == E_SHAPE and call(ncy=5) == E_SHAPE and call(ncx=2) == E_SHAPE and call(fnx=0) == E_SHAPE
        assert call(work=None) == E_WORKSPACE and call(wb=need - 1) == E_WORKSPACE
    assert b'spx_background_workspace_bytes' in lib.spx_last_error()


def test_estimate_background_argument_errors():
    from subpixal_amd import detect
    f = np.zeros((40, 50), np.float32)
    for box in ((7, 8), (8, 129), 64, (8.5, 8)):
        with pytest.raises(ValueError, match='box'):
            detect.estimate_background(f, box=box)
    with pytest.raises(ValueError, match='8192'):
        detect.estimate_background(f.astype(np.float64), box=(128, 128))
    with pytest.raises(ValueError, match='filter_size'):
        detect.estimate_background(f, filter_size=2)
    with pytest.raises(ValueError, match='mask'):
        detect.estimate_background(f, mask=np.zeros((8, 8), bool))
    with pytest.raises(ValueError, match='exclude'):
        detect.estimate_background(f, exclude=np.zeros((8, 8), np.int32))
    with pytest.raises(ValueError, match='int32'):
        detect.estimate_background(f, exclude=np.zeros(f.shape, np.int64))
    with pytest.raises(ValueError, match='sigma'):
        detect.estimate_background(f, sigma=0.0)
    with pytest.raises(ValueError, match='max_iters'):
        detect.estimate_background(f, max_iters=-1)
    with pytest.raises(ValueError, match='min_good_fraction'):
        detect.estimate_background(f, min_good_fraction=1.5)
    with pytest.raises(ValueError, match='2-D'):
        detect.estimate_background(np.zeros(8, np.float32))
    with pytest.raises(ValueError, match='passes'):
        detect.detect_sources(f, passes=3)
    with pytest.raises(TypeError, match='threshold'):
        detect.detect_sources(f, threshold=1.0)
    with pytest.raises(ValueError, match='box'):
        detect.detect_sources(f, box=(4, 4))
