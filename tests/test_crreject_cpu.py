"""Cosmic-ray rejection without a GPU: the two kernels of subpixal_amd/csrc/spx_crreject_kernels.h on CPU threads
(tests/cpu_emu/emu_crreject.cpp, rows packed and launched as spx_capi.hip does) against the numpy statement of
tests/crreject_statement.py on every case of tests/crreject_cases.py, in float32 and float64: `med` and `nmed`
exactly, `crmask` on every pixel whose decision is safe by the statement's bound, `clean` bit for bit off the mask and
within the blot bound on it; grid independence; every argument check of the four new C entries; the ValueErrors and
the mask bookkeeping of `resample.DeviceDrizzle`."""
import os
import re

import numpy as np
import pytest

import crreject_cases as cc
import crreject_emu as ce
import crreject_statement as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('spx_drizzle_median_f32', 'spx_drizzle_median_f64', 'spx_drizzle_cr_f32', 'spx_drizzle_cr_f64')
E_ARG, E_SHAPE = -1, -2
DTYPES = (np.float32, np.float64)


@pytest.fixture(scope='module')
def emuz(tmp_path_factory):
    return ce.load(tmp_path_factory)


def stated(lib, name, dtype):
    c = cc.ALL[name]()
    vals, valid = ce.singles(lib, c, dtype)
    return c, vals, valid, ce.statement(name, c, vals, valid, dtype)


# ---------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', sorted(cc.ALL))
def test_case_against_the_statement(emuz, name, dtype):
    c, vals, valid, st = stated(emuz, name, dtype)
    med, nmed = ce.run_median(emuz, c, dtype)
    assert med.dtype == np.float32 and nmed.dtype == np.uint8
    assert np.array_equal(nmed, st['nmed']), name
    assert med.tobytes() == st['med'].tobytes(), '%s: med differs at %d pixels' % (name, int((med != st['med']).sum()))
    if np.dtype(dtype) == np.float32:
        # item 1 without a second statement: np.sort over K single-frame runs of the existing drizzle harness
        act = np.array(ce.actives(c))[:, None, None]
        stack = np.where(valid & act, vals, np.inf)
        m = (valid & act).sum(axis=0)
        assert np.array_equal(nmed, m.astype(np.uint8))
        if not c['cr'].get('nlow') and not c['cr'].get('nhigh'):
            srt = np.sort(stack, axis=0)
            iy, ix = np.nonzero(m)
            mm = m[iy, ix]
            lo, hi = srt[(mm - 1) // 2, iy, ix], srt[mm // 2, iy, ix]
            exp = np.zeros(med.shape, np.float32)
            exp[iy, ix] = (0.5 * (lo.astype(np.float64) + hi.astype(np.float64))).astype(np.float32)
            exp[iy, ix] = np.where(mm % 2, lo, exp[iy, ix])
            assert med.tobytes() == exp.tobytes(), name
    tested = unsafe = 0
    for k, fs in enumerate(st['frames']):
        if fs is None:
            continue
        crmask, clean = ce.run_cr(emuz, c, dtype, k, med, nmed)
        unsafe += cs.check_frame(crmask, clean, c['frames'][k], fs, dtype, '%s frame %d' % (name, k))
        tested += int(fs['testable'].sum())
    assert unsafe <= 0.01 * tested, (name, unsafe, tested)


@pytest.mark.parametrize('name', sorted(cc.ALL))
def test_the_statement_alone_leaves_under_one_percent_undecided(name):
    """with the single-frame values of the scatter (no kernel anywhere): at most 1 % of a case's tested pixels have a
    decision margin under the bound"""
    c = cc.ALL[name]()
    st = cs.statement(c, *cs.singles_by_scatter(c))
    tested = sum(int(f['testable'].sum()) for f in st['frames'] if f is not None)
    unsafe = sum(int((~f['safe'] & f['testable']).sum()) for f in st['frames'] if f is not None)
    print('%s: %d tested, %d under the bound' % (name, tested, unsafe))
    assert tested > 0 and unsafe <= 0.01 * tested


def test_the_cases_cover_what_they_claim(emuz):
    for name, fn in cc.ALL.items():
        c = fn()
        assert all(5 <= min(f.shape) and max(f.shape) <= 33 for f in c['frames']), name
        assert c['out_shape'][0] % 8 and c['out_shape'][1] % 32, name
    flagged, keep = {}, {}
    for name in ('k3_hits', 'positions', 'neighbour_rule', 'rms_map_nan', 'half_outside', 'many33', 'k4_nhigh',
                 'fallback', 'fallback_partly', 'inactive_middle'):
        c, vals, valid, st = stated(emuz, name, np.float32)
        flagged[name] = {(k, j, i): bool(st['frames'][k]['crmask'][j, i]) for k, j, i, a in c['hits']
                         if st['frames'][k] is not None}
        keep[name] = (c, st)
    assert all(flagged['k3_hits'].values())
    # a frame corner, both sides of a tile boundary, next to a masked pixel and next to a NaN: flagged; on a
    # zero-weight pixel: not flagged
    assert flagged['positions'] == {(0, 0, 0): True, (0, 8, 32): True, (0, 7, 31): True, (0, 7, 32): True,
                                    (0, 8, 31): True, (1, 3, 10): True, (1, 5, 20): True, (2, 4, 15): False}
    c, st = keep['positions']
    assert c['masks'][1][3, 11] and np.isnan(c['frames'][1][5, 21]) and c['weights'][2][4, 15] == 0
    # the neighbour rule: the fainter pixel passes test 1, fails test 2 and is flagged; the isolated one is not
    f = keep['neighbour_rule'][1]['frames'][0]
    assert f['fail'][0][5, 10] and f['fail'][1][5, 10]
    assert not f['fail'][0][5, 11] and f['fail'][1][5, 11] and f['crmask'][5, 11]
    assert not f['fail'][0][8, 20] and f['fail'][1][8, 20] and not f['crmask'][8, 20]
    assert f['crmask'].sum() == 2
    # an rms that is NaN or negative under a hit: not testable, not flagged
    assert flagged['rms_map_nan'] == {(0, 3, 7): False, (1, 8, 20): False, (2, 6, 14): True, (0, 9, 25): True}
    # a band without a blot, hits in it and outside it
    f = keep['half_outside'][1]['frames'][0]
    assert 0.2 < f['defined'].mean() < 0.8 and flagged['half_outside'][0, 20, 25] and not flagged['half_outside'][0, 2, 3]
    assert keep['many33'][1]['nmed'].max() == 33 and len(keep['many33'][0]['frames']) == 33
    # nhigh = 1 changes the median; the fallback leaves pixels with m <= nlow + nhigh untrimmed
    c, st = keep['k4_nhigh']
    vals, valid = ce.singles(emuz, c, np.float32)
    assert (cs.median(vals, valid)[0] != st['med']).any()
    c, st = keep['fallback']
    vals, valid = ce.singles(emuz, c, np.float32)
    assert st['nmed'].max() == 2 and cs.median(vals, valid)[0].tobytes() == st['med'].tobytes()
    nm = keep['fallback_partly'][1]['nmed']
    assert (nm == 3).any() and (nm == 2).any() and (nm == 1).any()
    assert keep['inactive_middle'][1]['frames'][1] is None and flagged['inactive_middle'] == {(0, 5, 5): True,
                                                                                              (2, 7, 17): True}


@pytest.mark.parametrize('dtype', DTYPES)
def test_grid_size_does_not_matter_and_runs_are_identical(emuz, dtype):
    for name in ('many33', 'geometry', 'narrow', 'positions'):
        c = cc.ALL[name]()
        meds = [ce.run_median(emuz, c, dtype, grid=g) for g in (0, 1, 3, 0)]
        for r in meds[1:]:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(r, meds[0])), name
        for k in range(min(len(c['frames']), 4)):
            runs = [ce.run_cr(emuz, c, dtype, k, *meds[0], grid=g) for g in (0, 1, 2, 0)]
            for r in runs[1:]:
                assert all(a.tobytes() == b.tobytes() for a, b in zip(r, runs[0])), (name, k)


def test_every_output_element_is_written(emuz):
    for name in ('narrow', 'half_outside', 'k1'):
        c = cc.ALL[name]()
        med, nmed = ce.run_median(emuz, c, np.float32)
        assert not (med == -77).any() and not (nmed == 201).any(), name
        for k in range(len(c['frames'])):
            crmask, clean = ce.run_cr(emuz, c, np.float32, k, med, nmed)
            assert crmask.max() <= 1 and not (clean == -77).any(), (name, k)


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
    assert 'UNPINNED' in header[header.index('Cosmic-ray rejection for the drizzle'):]
    table = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in ('spx_drizzle_median_f32', 'spx_drizzle_cr_f32'):
        assert '`%s`' % name in table, name


def test_c_argument_errors_of_the_median_before_any_hip_call():
    from subpixal_amd import _ffi
    lib = _ffi.load()
    buf = np.zeros(64, np.float64)
    b = buf.ctypes.data
    for fn in (lib.spx_drizzle_median_f32, lib.spx_drizzle_median_f64):
        def call(rows=b, K=2, nact=2, kernel=0, nlow=0, nhigh=0, ny=4, nx=4, med=b, nmed=b):
            return fn(rows, K, nact, kernel, nlow, nhigh, ny, nx, med, nmed, None)
        for name in ('rows', 'med', 'nmed'):
            assert call(**{name: None}) == E_ARG and b'null' in lib.spx_last_error(), name
        for kw in (dict(K=0), dict(K=129), dict(K=-1), dict(nact=0), dict(nact=3), dict(nact=-1), dict(kernel=3),
                   dict(kernel=-1), dict(nlow=-1), dict(nhigh=-1)):
            assert call(**kw) == E_ARG, kw
            assert lib.spx_last_error()
        for kw in (dict(ny=0), dict(nx=-1), dict(ny=65536, nx=32768)):
            assert call(**kw) == E_SHAPE, kw
    assert not buf.any()


def test_c_argument_errors_of_the_comparison_before_any_hip_call():
    from subpixal_amd import _ffi
    lib = _ffi.load()
    buf = np.zeros(64, np.float64)
    b = buf.ctypes.data
    nan, inf = float('nan'), float('inf')
    for fn in (lib.spx_drizzle_cr_f32, lib.spx_drizzle_cr_f64):
        def call(rows=b, K=2, frame=1, fny=5, fnx=5, med=b, nmed=b, ny=8, nx=8, rms=0.1, rms_map=None, sky=0.0,
                 gain=nan, snr1=3.5, snr2=3.0, scale1=1.2, scale2=0.7, crmask=b, clean=b):
            return fn(rows, K, frame, fny, fnx, med, nmed, ny, nx, rms, rms_map, sky, gain, snr1, snr2, scale1, scale2,
                      crmask, clean, None)
        for name in ('rows', 'med', 'nmed', 'crmask', 'clean'):
            assert call(**{name: None}) == E_ARG and b'null' in lib.spx_last_error(), name
        for kw in (dict(K=0), dict(K=129), dict(frame=-1), dict(frame=2), dict(snr1=nan), dict(snr1=inf),
                   dict(snr2=-1.0), dict(scale1=nan), dict(scale1=inf), dict(scale2=-0.5), dict(snr2=nan),
                   dict(scale2=nan), dict(snr1=2.0, snr2=3.0), dict(scale1=0.5, scale2=0.7), dict(sky=nan)):
            assert call(**kw) == E_ARG, kw
            assert lib.spx_last_error()
        for kw in (dict(fny=0), dict(fnx=-1), dict(fny=65536, fnx=32768), dict(ny=0), dict(nx=-1),
                   dict(ny=65536, nx=32768), dict(ny=5), dict(nx=5)):
            assert call(**kw) == E_SHAPE, kw
    assert not buf.any()


# ---------------------------------------------------------------------------------------------------------------
# resample.DeviceDrizzle, host side only
# ---------------------------------------------------------------------------------------------------------------
def _host_drizzle(K=3, **kw):
    from subpixal_amd import resample
    frames = [np.zeros((6, 7), np.float32) for _ in range(K)]
    a = dict(frames=frames, maps=np.tile([1.0, 0, 0, 0, 1, 0], (K, 1)), out_shape=(9, 10),
             names=['a', 'b', 'c', 'd', 'e'][:K])
    a.update(kw)
    return resample.DeviceDrizzle(**a)


def test_python_argument_errors_before_the_device():
    m = np.full((6, 7), 0.1, np.float32)
    for kw, what in ((dict(cr_reject=True), 'rms'), (dict(cr_reject=True, rms=[0.1, 0.1]), 'rms'),
                     (dict(cr_reject=True, rms=[0.1, np.zeros((6, 6), np.float32), 0.1]), 'rms'),
                     (dict(cr_reject=True, rms=0.1, gain=[1.0, 2.0]), 'gain'),
                     (dict(cr_reject=True, rms=0.1, gain=[1.0, m, 2.0]), 'gain'),
                     (dict(cr_reject=True, rms=0.1, sky=float('nan')), 'sky'),
                     (dict(cr_reject=True, rms=0.1, sky=[0.0]), 'sky'),
                     (dict(cr_reject=True, rms=0.1, combine_nlow=-1), 'combine_nlow'),
                     (dict(cr_reject=True, rms=0.1, combine_nhigh=1.5), 'combine_nhigh'),
                     (dict(cr_reject=True, rms=0.1, driz_cr_snr=(3.0, 3.5)), 'driz_cr_snr'),
                     (dict(cr_reject=True, rms=0.1, driz_cr_snr=3.0), 'driz_cr_snr'),
                     (dict(cr_reject=True, rms=0.1, driz_cr_scale=(1.0, float('nan'))), 'driz_cr_scale'),
                     (dict(cr_reject=True, rms=0.1, driz_cr_scale=(-1.0, -2.0)), 'driz_cr_scale'),
                     (dict(cr_reject=True, rms=0.1, out_shape=(5, 10)), 'out_shape')):
        with pytest.raises(ValueError, match=what):
            _host_drizzle(**kw)
    d = _host_drizzle()
    assert d.output_crclean is None and d.output_crmask is None and d.output_median is None
    assert d.crclean('a') is None and d.crmask('a') is None
    with pytest.raises(ValueError, match='rms'):
        d.set_config_parameters(cr_reject=True)
    assert d._cr['on'] is False                                  # a refused call changes nothing
    d.set_config_parameters(cr_reject=True, rms=[0.1, m, 0.2], gain=2.0, sky=[0.0, 0.1, 0.2], combine_nhigh=1)
    assert d._cr['on'] and d._cr['rms']['a'] == 0.1 and d._cr['rms']['b'] is m and d._cr['gain'] == dict(a=2, b=2, c=2)
    assert d._cr['sky']['c'] == 0.2 and d._cr['nhigh'] == 1 and d._cr['snr'] == (3.5, 3.0) and d._cr['scale'] == (1.2, 0.7)
    d.set_config_parameters(cr_reject=False)
    assert d._cr['on'] is False and d._cr['rms']['a'] == 0.1
    # rms given, feature off: accepted and unused
    assert _host_drizzle(rms=0.1).output_crclean is None


class _FakeMask(object):
    """stands in for a resident mask tensor: only data_ptr() is asked of it"""
    def __init__(self, ptr):
        self.ptr = ptr

    def data_ptr(self):
        return self.ptr


def _packed_mask_pointers(d, names, **kw):
    """the mask pointers `_pack` hands to spx_drizzle_rows, without a device: frames made 'resident' as numpy arrays
    wrapped to have data_ptr()"""
    class Res(object):
        def __init__(self, a, ptr):
            self.shape, self.ptr = a.shape, ptr

        def data_ptr(self):
            return self.ptr
    for q, n in enumerate(d._order):
        f = d._pool[n]
        if not f.resident:
            f.data, f.resident = Res(f.data, 4096 * (q + 1)), True
            f.mask = None if f.mask is None else _FakeMask(100 + q)
    rows = d._pack(names, **kw)
    return [int(r[16:24].view(np.uint64)[0]) for r in rows]


def test_fast_replace_reuses_the_merged_masks_and_a_full_execute_starts_from_the_originals():
    masks = [np.zeros((6, 7), np.uint8), None, None, None]
    d = _host_drizzle(K=4, masks=masks, cr_reject=True, rms=0.1)
    full = []

    def fake_reject(lib):                                          # what _reject_cosmic_rays leaves behind
        full.append(list(d.input_image_names))
        gen = len(full)
        d._crmask = {n: _FakeMask(1000 * gen + k) for k, n in enumerate(d.input_image_names)}
        d._merged = {n: _FakeMask(2000 * gen + k) for k, n in enumerate(d.input_image_names)}
        d._crclean = {n: 'clean %s %d' % (n, gen) for n in d.input_image_names}
    d._reject_cosmic_rays = fake_reject
    # before any full execute(): the original masks
    assert _packed_mask_pointers(d, ['a', 'b']) == [100, 0]
    d._fast = False
    fake_reject(None)
    assert _packed_mask_pointers(d, ['a', 'b', 'c', 'd']) == [2000, 2001, 2002, 2003]
    assert _packed_mask_pointers(d, ['a', 'b'], original=True) == [100, 0]
    # a fast replace runs execute() with the steps switched off and keeps the masks
    runs = []
    d.execute = lambda: runs.append((d._fast, list(d.input_image_names)))
    d.fast_drop_image('b')
    assert runs == [(True, ['a', 'c', 'd'])] and d._fast is False and len(full) == 1
    assert _packed_mask_pointers(d, d._order) == [2000, 2001, 2002, 2003]
    # a copy carries the masks and the clean frames along, in dicts of its own
    q = d.copy()
    assert q.crclean('c') == 'clean c 1' and q.crmask('a') is d.crmask('a') and q._merged is not d._merged
    q._merged.pop('a')
    assert _packed_mask_pointers(q, ['a']) == [100]    # no CR mask: the original mask
    assert _packed_mask_pointers(d, ['a']) == [2000]
    # the next full execute() makes new masks
    fake_reject(None)
    assert _packed_mask_pointers(d, ['a', 'c', 'd']) == [4000, 4001, 4002] and d.crclean('b') is None
    # with the feature off the original masks are packed whatever is stored
    d.set_config_parameters(cr_reject=False)
    assert _packed_mask_pointers(d, ['a', 'c']) == [100, 0]


def test_nothing_listed_nothing_rejected():
    """a full execute() with every frame dropped: the rejection is skipped before any launch"""
    d = _host_drizzle(K=2, cr_reject=True, rms=0.1)
    d._crmask, d._merged, d._crclean = dict(a=1), dict(a=2), dict(a=3)
    d._active = dict(a=False, b=False)
    d._reject_cosmic_rays(None)
    assert d.input_image_names == [] and d.output_crmask == [] and d.output_crclean == []
    assert d.output_median is None and d.output_nmedian is None
    assert d.crmask('a') is None and d.crclean('a') is None and not d._merged and d._stale


class _StubDrizzle(object):
    """what align._frame_catalogs asks of a leave-one-out drizzle, on the host"""
    reference_image = (40, 40)

    def __init__(self, frame, clean):
        self.frame, self.clean = frame, clean
        self.output_sci = np.zeros((40, 40), np.float32)
        self.output_wht = np.ones((40, 40), np.float32)

    def map(self, name):
        return np.array([1.0, 0.0, 2.0, 0.0, 1.0, 3.0])

    def _resident(self, name):
        return type('Res', (object,), dict(data=self.frame))()

    def crclean(self, name):
        return self.clean


def test_frame_catalogs_cuts_from_the_cleaned_frame(monkeypatch):
    import inspect
    from subpixal_amd import align, cutout
    made = []

    class Recorder(object):                                        # the catalogs, without a device
        def __init__(self, frame, boxes, **kw):
            self.frame, self.boxes = frame, np.asarray(boxes)
            made.append(self)

        def pixels(self):
            return [self.frame[y:y + h, x:x + w] for x, y, w, h in self.boxes]
    monkeypatch.setattr(cutout, 'CutoutCatalog', Recorder)
    rng = np.random.default_rng(5)
    frame = rng.normal(size=(30, 32)).astype(np.float32)
    clean = frame.copy()
    clean[12, 11] = 7.0                                            # a rejected pixel inside the first source's box
    clean[2, 30] = -7.0                                            # and one in no box
    prim = type('Prim', (object,), dict(boxes=np.array([[10, 12, 7, 7], [22, 20, 5, 6]], np.int32),
                                        src_pos=np.array([[13.0, 15.0], [24.0, 22.5]]), src_weight=None,
                                        src_id=np.array([1, 2], np.int32), segmentation_image=None))()
    for cl in (clean, None):
        del made[:]
        align._frame_catalogs(_StubDrizzle(frame, cl), 'a', prim, 2, np.float32)
        img = made[0]
        assert img.boxes.tolist() == [[8, 9, 7, 7], [20, 17, 5, 6]]       # the primary boxes through M^-1
        src = frame if cl is None else cl
        for got, (x, y, w, h) in zip(img.pixels(), img.boxes):
            assert got.tobytes() == src[y:y + h, x:x + w].tobytes()
        assert (img.pixels()[0][3, 3] == 7.0) == (cl is not None)          # frame pixel (11, 12) of the first cutout
        assert made[1].frame.shape == (40, 40)                            # the drizzled cutouts: the drizzle, as before
    assert list(inspect.signature(align._frame_catalogs).parameters) == ['q', 'name', 'prim', 'margin', 'dtype']
