"""Deblending without a GPU: the kernels of subpixal_amd/csrc/spx_deblend_kernels.h on CPU threads
(tests/cpu_emu/emu_deblend.cpp, launched as spx_capi.hip launches them) against the numpy/scipy statement of
tests/deblend_statement.py with EXACT equality of labels, parent and dflags; the new C entries' argument checks;
the ValueErrors of `detect.deblend` and `detect.find_sources`.

The statement's figures for the scenes (how many segments, which parents split) are asserted too: they are what
the definition gives for these scenes, worked out with the statement alone.  SPX_EMU_DEBLEND_LIB: a pre-built
harness."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import deblend_cases as dc
import deblend_statement as dst

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'subpixal_amd', 'csrc')
NEW = ('spx_deblend_workspace_bytes', 'spx_deblend_labels_f32', 'spx_deblend_labels_f64')
E_ARG, E_SHAPE, E_WORKSPACE = -1, -2, -4
_LIB = {}
_ST = {}                                         # statements, computed once per scene and shared


@pytest.fixture(scope='module')
def emub(tmp_path_factory):
    if 'lib' not in _LIB:
        so = os.environ.get('SPX_EMU_DEBLEND_LIB')
        if not so:
            out = subprocess.check_output(['make', '-s', '-C', CSRC, '--eval',
                                           'spx-emu-flags: ; @echo $(HOSTCXX) $(EMUFLAGS)', 'spx-emu-flags'],
                                          universal_newlines=True).split()
            so = str(tmp_path_factory.mktemp('emub') / 'libspx_emu_deblend.so')
            subprocess.check_call(out + ['-shared', '-o', so, os.path.join(ROOT, 'tests', 'cpu_emu', 'emu_deblend.cpp')])
        lib = ctypes.CDLL(so)
        for fn in (lib.emub_deblend_f32, lib.emub_deblend_f64):
            fn.argtypes = ([ctypes.c_void_p] * 3 + [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
                           + [ctypes.c_int] * 3 + [ctypes.c_double, ctypes.c_int] + [ctypes.c_void_p] * 3
                           + [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int])
        _LIB['lib'] = lib
    return _LIB['lib']


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _args(s, dtype, over):
    kw = dict(levels_n=31, contrast=0.005, mode='exponential', min_area=5, conn=8)
    kw.update(s['kw'])
    kw.update(over)
    frame = np.ascontiguousarray(s['frame'], dtype)
    labels, n = dc.label_np(frame, s['thr'], s['mask'], s['filt'], kw['min_area'], kw['conn'])
    return frame, labels, n, kw


def run_emu(lib, s, dtype=np.float32, grid=3, lds_pixels=None, max_out=None, **over):
    frame, labels, n, kw = _args(s, dtype, over)
    ny, nx = frame.shape
    m = None if s['mask'] is None else np.ascontiguousarray(s['mask'], np.uint8)
    k = None if s['filt'] is None else np.ascontiguousarray(s['filt'], dtype)
    fky, fkx = (1, 1) if k is None else k.shape
    boxes = dc.bboxes_np(labels, n)
    max_out = ny * nx // kw['min_area'] + 1 if max_out is None else max_out
    out = np.full((ny, nx), -5, np.int32)
    parent = np.full(max_out, -5, np.int32)
    dflags = np.full(max_out, -5, np.int32)
    nout = np.full(1, -5, np.int32)
    fn = lib.emub_deblend_f64 if dtype == np.float64 else lib.emub_deblend_f32
    lab = np.ascontiguousarray(labels, np.int32)
    assert fn(_p(frame), _p(m), _p(k), fky, fkx, ny, nx, _p(lab), n, _p(boxes), kw['conn'], kw['min_area'],
              kw['levels_n'], kw['contrast'], dst.MODES[kw['mode']], _p(out), _p(parent), _p(dflags), max_out,
              _p(nout), grid, lib.emub_lds_pixels() if lds_pixels is None else lds_pixels) == 0
    return out, int(nout[0]), parent, dflags


def state(s, name, dtype=np.float32, **over):
    key = (name, np.dtype(dtype).name, tuple(sorted(over.items())))
    if key not in _ST:
        frame, labels, n, kw = _args(s, dtype, over)
        st = dst.statement(frame, labels, n, mask=s['mask'], filt=s['filt'], **kw)
        st['nparents'] = n
        for a in st.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _ST[key] = st
    return _ST[key]


def both(lib, s, name, dtype=np.float32, **over):
    st = state(s, name, dtype, **over)
    got = run_emu(lib, s, dtype, **over)
    dst.check(*got, st, what=name)
    print('%s %s: %d parents -> %d segments, split %s' % (name, np.dtype(dtype).name, st['nparents'], st['n'],
                                                          st['split']))
    return st


DTYPES = (np.float32, np.float64)


# ---------------------------------------------------------------------------------------------------------------
# splitting and the tree
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('sep,ratio,nparents,nseg', [(6, 1.0, 1, 1), (8, 1.0, 1, 2), (12, 1.0, 1, 2), (12, 0.1, 1, 2),
                                                     (8, 0.1, 1, 1), (12, 0.01, 2, 2), (8, 0.01, 1, 1)])
def test_gaussian_pairs_on_both_sides_of_splitting(emub, sep, ratio, nparents, nseg, dtype):
    """(at 12 px the 1 : 0.01 companion is a detection of its own, at 8 px it sits inside the bright star's
    isophote: it never splits off either way)"""
    st = both(emub, dc.pair(sep, ratio), 'pair %d %g' % (sep, ratio), dtype)
    assert st['nparents'] == nparents and st['n'] == nseg
    assert list(st['dflags']) == ([dst.FLAG_DEBLENDED] * 2 if nseg > nparents else [0] * nseg)


@pytest.mark.parametrize('levels,nseg', [(31, 3), (7, 3), (1, 2)])
def test_nested_triple(emub, levels, nseg):
    """the junction that inherits objs from one child (the 100 / 60 pair) and takes a bare candidate from the other"""
    st = both(emub, dc.triple(), 'triple', levels_n=levels)
    assert st['nparents'] == 1 and st['n'] == nseg


def _branch_records(s, y, x, **over):
    """the statement's tree records of the children that hold frame pixel (y, x), highest level first"""
    frame, labels, n, kw = _args(s, np.float32, over)
    trace = {}
    dst.statement(frame, labels, n, mask=s['mask'], filt=s['filt'], trace=trace, **kw)
    y0, x0, rec = trace[int(labels[y, x])]
    out = []
    for r in rec:
        if r['mask'][y - y0, x - x0]:
            full = np.zeros(labels.shape, bool)
            full[y0:y0 + r['mask'].shape[0], x0:x0 + r['mask'].shape[1]] = r['mask']
            out.append(dict(r, mask=full))                       # the mask in frame coordinates
    return out


def test_weak_bump_goes_to_its_neighbour_by_the_flood(emub):
    s = dc.weak_bump()
    st = both(emub, s, 'weak bump')
    assert st['nparents'] == 1 and st['n'] == 2
    assert st['labels'][dc.BUMP] == st['labels'][21, 20]         # the bump belongs to the star it sits on
    # ... because it never counted: while it is a branch of its own (the star's peak is not in it) it is
    # insignificant at every level, its own first level included
    own = [r for r in _branch_records(s, *dc.BUMP) if not r['mask'][21, 20]]
    assert own and own[0]['npix'] >= 1 and not any(r['significant'] for r in own)
    assert all(r['share'] < 0.005 or r['npix'] < 5 for r in own)


def test_candidate_significant_only_further_down(emub):
    s = dc.late_bloomer()
    st = both(emub, s, 'late bloomer')
    assert st['nparents'] == 1 and st['n'] == 2
    # the faint star's branch, while the bright star (27, 24) is not in it: insignificant where it first appears
    # (too few pixels or too little flux), significant at a lower level, without objects of its own throughout
    own = [r for r in _branch_records(s, 27, 37) if not r['mask'][27, 24]]
    assert len(own) >= 2 and not any(r['has_objs'] for r in own)
    assert not own[0]['significant'] and (own[0]['npix'] < 5 or own[0]['share'] < 0.005)
    assert own[-1]['significant'] and own[-1]['npix'] >= 5 and own[-1]['share'] >= 0.005
    assert own[0]['level'] > own[-1]['level']
    # with one level only (at half the range) the faint star is not above it at all: nothing to split
    assert both(emub, s, 'late bloomer', levels_n=1)['n'] == 1


# ---------------------------------------------------------------------------------------------------------------
# ties and refusals
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('conn', (8, 4))
@pytest.mark.parametrize('mode', ('exponential', 'linear'))
def test_plateaus_tie_break_to_the_smaller_object(emub, mode, conn):
    s = dc.plateaus()
    st = both(emub, s, 'plateaus', mode=mode, conn=conn)
    assert st['n'] == 2
    lab = st['labels']
    # the bridge's middle pixel is reached by both in the same sweep with equal q: it goes to object 1 (the left)
    assert lab[7, 12] == lab[7, 6] and lab[7, 13] == lab[7, 18]
    both(emub, s, 'plateaus', np.float64, mode=mode, conn=conn)


def test_flat_parent_is_left_whole(emub):
    st = both(emub, dc.flat(), 'flat')
    assert st['n'] == 1 and list(st['dflags']) == [0]


@pytest.mark.parametrize('dtype', DTYPES)
def test_exponential_mode_with_lo_not_positive_takes_linear_levels(emub, dtype):
    s = dc.pair(12, 1.0)
    frame, labels, n, kw = _args(s, dtype, {})
    shifted = dict(s, frame=s['frame'] - 8.0)

    def run(mode):
        fr = np.ascontiguousarray(shifted['frame'], dtype)
        st = dst.statement(fr, labels, n, filt=s['filt'], **dict(kw, mode=mode))
        k = np.ascontiguousarray(s['filt'], dtype)
        ny, nx = fr.shape
        out = np.full((ny, nx), -5, np.int32)
        parent = np.full(64, -5, np.int32)
        dflags = np.full(64, -5, np.int32)
        nout = np.full(1, -5, np.int32)
        fn = emub.emub_deblend_f64 if dtype == np.float64 else emub.emub_deblend_f32
        assert fn(_p(fr), None, _p(k), 3, 3, ny, nx, _p(labels), n, _p(dc.bboxes_np(labels, n)), 8, 5, 31, 0.005,
                  dst.MODES[mode], _p(out), _p(parent), _p(dflags), 64, _p(nout), 3, emub.emub_lds_pixels()) == 0
        dst.check(out, int(nout[0]), parent, dflags, st, what='shifted ' + mode)
        return out
    assert dst.filtered(shifted['frame'], None, s['filt'])[labels > 0].min() < 0
    assert np.array_equal(run('exponential'), run('linear'))
    assert dst.levels(-1.0, 3.0, 31, 0) == dst.levels(-1.0, 3.0, 31, 1) == [k << 25 for k in range(32)]


def test_seed_smaller_than_min_area(emub):
    s = dc.needles()
    assert both(emub, s, 'needles')['n'] == 1                   # 1-pixel branches: never significant
    assert both(emub, s, 'needles', min_area=1)['n'] == 2


# ---------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_parents_in_the_corners_with_a_wide_filter(emub, dtype):
    st = both(emub, dc.corners(), 'corners', dtype)
    assert st['nparents'] == 4 and st['n'] == 8


def test_masked_pixel_inside_a_parent(emub):
    st = both(emub, dc.masked(), 'masked')
    assert st['n'] == 2


def test_ring_with_other_parents_inside_its_box(emub):
    st = both(emub, dc.ring(), 'ring')
    assert st['nparents'] == 3 and 1 in st['split'] and st['n'] >= 5
    both(emub, dc.ring(), 'ring', conn=4)


def test_box_over_the_limit_is_flagged_and_left_whole(emub):
    s = dc.big_ring()
    st = both(emub, s, 'big ring')
    assert st['nparents'] == 2 and st['n'] == 3
    assert sorted(st['dflags']) == [dst.FLAG_DEBLENDED] * 2 + [dst.FLAG_NODEBLEND]
    labels, _ = dc.label_np(s['frame'], s['thr'], None, None, 1, 8)
    assert np.array_equal(st['labels'] == 1, labels == 1)       # the ring's pixels, renumbered at most


def test_large_blob_takes_the_workspace_and_small_one_lds(emub):
    big, small = dc.blob(150), dc.blob(40)
    for s, lds in ((big, False), (small, True)):
        labels, n = dc.label_np(s['frame'], s['thr'], None, None, 5, 8)
        b = dc.bboxes_np(labels, n)[1]
        assert n == 1 and ((b[2] - b[0] + 1) * (b[3] - b[1] + 1) <= emub.emub_lds_pixels()) == lds
    stb = both(emub, big, 'blob 150')
    sts = both(emub, small, 'blob 40')
    assert stb['n'] == sts['n'] == 3
    # the small one again through the workspace path and through the one-wave path's neighbour class: the storage
    # a parent took must not matter
    got = run_emu(emub, small, lds_pixels=1024)
    dst.check(*got, sts, what='blob 40 through the workspace')


# ---------------------------------------------------------------------------------------------------------------
# numbering and invariants
# ---------------------------------------------------------------------------------------------------------------
def test_children_of_different_parents_interleave(emub):
    st = both(emub, dc.interleaved(), 'interleaved')
    assert list(st['parent']) == [1, 2, 1, 2] and list(st['dflags']) == [8] * 4


@pytest.mark.parametrize('conn', (8, 4))
@pytest.mark.parametrize('dtype', DTYPES)
def test_smooth_random_field(emub, dtype, conn):
    st = both(emub, dc.smooth_field(), 'smooth field', dtype, conn=conn)
    assert st['nparents'] >= 10 and 3 <= len(st['split']) <= st['nparents'] // 2


def test_rows_beyond_max_out_are_not_written(emub):
    s = dc.interleaved()
    st = state(s, 'interleaved')
    out, n, parent, dflags = run_emu(emub, s, max_out=3)
    assert n == st['n'] == 4 and np.array_equal(out, st['labels'])
    assert np.array_equal(parent, st['parent'][:3]) and np.array_equal(dflags, st['dflags'][:3])


def test_grid_size_does_not_matter_and_runs_are_identical(emub):
    s = dc.smooth_field()
    a = run_emu(emub, s, grid=1)
    b = run_emu(emub, s, grid=64)
    c = run_emu(emub, s, grid=64)
    for x, y, z in zip(a, b, c):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes() == np.asarray(z).tobytes()


def test_level_guard_and_level_arithmetic():
    """the statement's own pieces: linear levels are exact, exponential ones rise and end below 2^30, and the
    guard fires for an x_k that sits on an integer"""
    assert dst.levels(1.0, 2.0, 3, 1) == [0, 1 << 28, 1 << 29, 3 << 28]
    tq = dst.levels(1.5, 700.25, 31, 0)
    assert tq[0] == 0 and all(a < b for a, b in zip(tq, tq[1:])) and tq[-1] < 2 ** 30
    assert dst.levels(1.0, 4.0, 1, 0) == [0, -(-2 ** 30 // 3)]          # g = 2, x_1 = 2^30 / 3, rounded up
    with pytest.raises(AssertionError, match='1e-5'):
        dst.levels(1.0, 9.0, 1, 0)               # g = 3, x_1 = 2 / 8 * 2^30: an integer


def test_committed_scenes_stay_clear_of_the_level_guard():
    """every parent of every scene of deblend_cases.py (the GPU tests' ones included), at every number of levels
    the tests use: all x_k farther than 1e-5 from an integer.  A scene that trips this gets another seed."""
    scenes = {'pair %g %g' % (s, r): dc.pair(s, r) for s, r in ((6, 1.0), (8, 1.0), (12, 1.0), (12, 0.1), (8, 0.1),
                                                                 (12, 0.01), (8, 0.01))}
    scenes.update(triple=dc.triple(), weak_bump=dc.weak_bump(), late_bloomer=dc.late_bloomer(), plateaus=dc.plateaus(),
                  needles=dc.needles(), corners=dc.corners(), masked=dc.masked(), ring=dc.ring(), big_ring=dc.big_ring(),
                  blob150=dc.blob(150), blob40=dc.blob(40), interleaved=dc.interleaved(), field=dc.smooth_field(),
                  field_big=dc.smooth_field(seed=12, shape=(240, 300)), crowded=dc.crowded())
    worst, nparents = {}, 0
    for name, s in scenes.items():
        for conn in (8, 4):
            min_area = s['kw'].get('min_area', 5)
            labels, n = dc.label_np(s['frame'], s['thr'], s['mask'], s['filt'], min_area, conn)
            f = dst.filtered(s['frame'], s['mask'], s['filt'])
            for l in range(1, n + 1):
                v = f[labels == l]
                if not v.max() > v.min():
                    continue
                for nlev in (31, 7, 1):
                    margin = []
                    dst.levels(v.min(), v.max(), nlev, 0, margin)            # raises when the guard fires
                    worst[name] = min([worst.get(name, 1.0)] + margin)
                nparents += 1
    print('parents examined: %d; smallest distance of an x_k from an integer per scene: %s'
          % (nparents, ', '.join('%s %.1e' % kv for kv in sorted(worst.items()))))
    assert nparents > 300 and all(m > 1e-5 for m in worst.values())


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
    header = open(os.path.join(ROOT, 'include', 'subpixal_hip.h')).read()
    assert '#define SPX_DEBLEND_MAX_BOX_PIXELS 65536' in header
    table = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in ('spx_deblend_workspace_bytes', 'spx_deblend_labels_f32', '_f64'):
        assert '`%s`' % name in table, name


def test_c_argument_errors_before_any_hip_call():
    from subpixal_amd import _ffi
    lib = _ffi.load()
    buf = np.zeros(1024, np.float64)
    b = buf.ctypes.data
    need = lib.spx_deblend_workspace_bytes(8, 8, 3)
    assert need >= lib.spx_detect_workspace_bytes(8, 8) + 4 * 4
    assert lib.spx_deblend_workspace_bytes(0, 8, 3) == 0 and lib.spx_deblend_workspace_bytes(65536, 32768, 3) == 0
    assert lib.spx_deblend_workspace_bytes(8, 8, -1) == 0
    # a frame that can hold a parent beyond LDS needs slots: 36 B per pixel of the largest box, per slot
    assert (lib.spx_deblend_workspace_bytes(100, 100, 1) - lib.spx_deblend_workspace_bytes(100, 100, 0)
            >= 36 * 100 * 100)
    for fn in (lib.spx_deblend_labels_f32, lib.spx_deblend_labels_f64):
        def call(frame=b, filt=None, fky=1, fkx=1, fny=8, fnx=8, labels=b, nlabels=3, boxes=b, conn=8, min_area=5,
                 nlev=31, contrast=0.005, mode=0, work=b, wb=need, out=b, parent=b, dflags=b, max_out=4, nl=b):
            return fn(frame, None, filt, fky, fkx, fny, fnx, labels, nlabels, boxes, conn, min_area, nlev, contrast,
                      mode, work, wb, out, parent, dflags, max_out, nl, None)
        for name in ('frame', 'labels', 'boxes', 'out', 'parent', 'dflags', 'nl'):
            assert call(**{name: None}) == E_ARG, name
        assert call(conn=6) == E_ARG and call(conn=0) == E_ARG
        assert call(min_area=0) == E_ARG and call(nlabels=-1) == E_ARG and call(max_out=-1) == E_ARG
        for nlev in (0, 2, 4, 30, 32, 64, 127, -1):
            assert call(nlev=nlev) == E_ARG, nlev
        assert call(contrast=-0.001) == E_ARG and call(contrast=1.001) == E_ARG
        assert call(contrast=float('nan')) == E_ARG
        assert b'contrast' in lib.spx_last_error()
        assert call(mode=2) == E_ARG and call(mode=-1) == E_ARG
        assert call(filt=b, fky=2, fkx=3) == E_ARG and call(filt=b, fky=3, fkx=4) == E_ARG
        assert call(filt=b, fky=9, fkx=3) == E_ARG and call(filt=b, fky=3, fkx=9) == E_ARG
        assert call(fny=0) == E_SHAPE and call(fny=65536, fnx=32768) == E_SHAPE
        assert call(work=None) == E_WORKSPACE and call(wb=need - 1) == E_WORKSPACE
        for nlev in (1, 3, 7, 15, 31, 63):       # the legal ones get as far as the workspace check
            assert call(nlev=nlev, wb=0) == E_WORKSPACE, nlev


def test_python_argument_errors_before_the_device():
    from subpixal_amd import detect
    f = np.zeros((8, 9), np.float32)
    lab = np.zeros((8, 9), np.int32)
    for kw, what in ((dict(levels=30), 'levels'), (dict(levels=0), 'levels'), (dict(levels=127), 'levels'),
                     (dict(contrast=-0.1), 'contrast'), (dict(contrast=1.5), 'contrast'),
                     (dict(contrast=float('nan')), 'contrast'), (dict(mode='cubic'), 'mode'),
                     (dict(min_area=0), 'min_area'), (dict(connectivity=6), 'connectivity'),
                     (dict(filter_kernel=np.ones((2, 3))), 'odd'), (dict(mask=np.zeros((8, 8), bool)), 'mask')):
        with pytest.raises(ValueError, match=what):
            detect.deblend(f, lab, 0, **kw)
    with pytest.raises(ValueError, match='labels'):
        detect.deblend(f, np.zeros((8, 8), np.int32), 0)
    with pytest.raises(ValueError, match='nlabels'):
        detect.deblend(f, lab, -1)
    for kw, what in ((dict(deblend_levels=5), 'levels'), (dict(deblend_contrast=2.0), 'contrast'),
                     (dict(deblend_mode='log'), 'mode')):
        with pytest.raises(ValueError, match=what):
            detect.find_sources(f, 1.0, deblend=True, **kw)
        with pytest.raises(ValueError, match=what):
            detect.detect_sources(f, deblend=True, **kw)
    assert detect.FLAG_DEBLENDED == 8 and detect.FLAG_NODEBLEND == 16
