"""minmed and the mask growth without a GPU: the three kernels of subpixal_amd/csrc/spx_minmed_kernels.h on CPU threads
(tests/cpu_emu/emu_minmed.cpp, rows packed and launched as spx_capi.hip does) against the numpy statement of
tests/minmed_statement.py on every case of tests/minmed_cases.py, in float32 and float64, with EXACT equality (every
decision is float64 + - * / and comparisons); grid independence; every argument check of the four new C entries; the
new ValueErrors of `resample.DeviceDrizzle`; and the reason for the feature on a K = 2 scene."""
import inspect
import os
import re

import numpy as np
import pytest

import crreject_emu as ce
import crreject_statement as cs
import minmed_cases as mc
import minmed_emu as me
import minmed_statement as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('spx_drizzle_minmed_f32', 'spx_drizzle_minmed_f64', 'spx_drizzle_cr_grow_f32', 'spx_drizzle_cr_grow_f64')
E_ARG, E_SHAPE = -1, -2
DTYPES = (np.float32, np.float64)


@pytest.fixture(scope='module')
def emuz(tmp_path_factory):
    return me.load(tmp_path_factory)


_RUNS = {}


def combined(lib, name, dtype):
    """a COMBINE case, its single-frame values, the statement and the kernels' planes: computed once, read-only"""
    key = (name, np.dtype(dtype).name)
    if key not in _RUNS:
        c = mc.COMBINE[name]()
        vals, valid = ce.singles(lib, c, dtype)
        p, q = ce.params(c), me.mm_params(c)
        act = np.array(ce.actives(c))[:, None, None]
        st = ms.minmed(vals, valid & act, ms.table_of(c), q['nsigma'], q['grow'], p['nlow'], p['nhigh'])
        _RUNS[key] = (c, st, me.run_minmed(lib, c, dtype))
    return _RUNS[key]


# ---------------------------------------------------------------------------------------------------------------
# step 2'
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', sorted(mc.COMBINE))
def test_minmed_case_equals_the_statement(emuz, name, dtype):
    c, st, got = combined(emuz, name, dtype)
    assert got['med'].dtype == np.float32 and got['nmed'].dtype == np.uint8 and got['minmed'].dtype == np.uint8
    assert np.array_equal(got['nmed'], st['nmed']), name
    assert np.array_equal(got['minmed'], st['minmed']), \
        '%s: output_minmed differs at %d pixels' % (name, int((got['minmed'] != st['minmed']).sum()))
    assert got['med'].tobytes() == st['med'].tobytes(), name
    assert got['lo'].tobytes() == st['lo'].tobytes(), name
    assert np.array_equal(got['bits'], st['hit'][0] + 2 * st['hit'][1]), name
    # md is the EXISTING median kernel's med on the same case, bit for bit
    med, nmed = ce.run_median(emuz, c, dtype)
    assert got['md'].tobytes() == med.tobytes() and np.array_equal(got['nmed'], nmed), name


def test_the_combine_cases_cover_what_they_claim(emuz):
    seen = {}
    for name in sorted(mc.COMBINE):
        c, st, got = combined(emuz, name, np.float32)
        seen[name] = (c, st)
        if name != 'many65':
            assert c['out_shape'] == (45, 70), name
    assert {len(seen[n][0]['frames']) for n in seen} >= {2, 3, 5, 65}
    assert seen['many65'][1]['nmed'].max() == 65                 # a column of 65 x 1024 bytes of LDS
    assert seen['many65'][1]['minmed'].any()
    for name in ('k2', 'k3_gain', 'k5_trim', 'k3_inactive_weight', 'small_frames'):
        how = seen[name][1]['minmed']
        assert (how == 1).any() and (how == 0).any(), name
    # the neighbour rule: seeds at x = 31 | 32, y = 7 | 8, on the border and in a corner; faint pixels at distance 1,
    # 8 and 9 of a seed, and one far from any
    for grow, by_rule in ((0, set()), (1, {(7, 32), (8, 31), (6, 30), (1, 21), (43, 68)}),
                          (8, {(7, 32), (8, 31), (6, 30), (1, 21), (43, 68), (16, 40), (15, 23), (30, 58), (22, 42),
                               (28, 0)})):
        st = seen['planted_grow%d' % grow][1]
        assert {tuple(p) for p in np.argwhere(st['minmed'] == 1)} == set(mc.SEEDS), grow
        assert {tuple(p) for p in np.argwhere(st['minmed'] == 2)} == by_rule, grow
        assert {tuple(p) for p in np.argwhere(st['hit'][1] & ~st['hit'][0])} == set(mc.FAINT)
    # ties: the minimum comes from rows 1 and 2; only kmin = 1 (combine_rms 0.01) makes the hit pixels seeds
    c, st = seen['ties']
    assert {tuple(p) for p in np.argwhere(st['minmed'] == 1)} == set(mc.SEEDS)
    assert all(st['kmin'][y, x] == 1 for y, x in mc.SEEDS)
    assert not ms.minmed(*ce.singles(emuz, c, np.float32), np.roll(ms.table_of(c), 1, axis=0))['minmed'].any()
    # m = 0, 1, 2, 3 pixels; an inactive row's hit is not seen; gain absent and present; trimming
    assert set(np.unique(seen['small_frames'][1]['nmed'])) >= {0, 1, 2, 3}
    c, st = seen['k3_inactive_weight']
    assert c['active'] == [1, 0, 1, 1] and st['nmed'].max() == 3 and float(st['med'].max()) < 20
    assert ms.table_of(seen['k3_gain'][0])[0, 2] == 400.0 and ms.table_of(seen['k2'][0])[0, 2] == 0.0
    c, st = seen['k5_trim']
    assert (cs.median(*ce.singles(emuz, c, np.float32))[0] != st['md']).any()


@pytest.mark.parametrize('dtype', DTYPES)
def test_minmed_does_not_depend_on_the_grid(emuz, dtype):
    for name in ('planted_grow8', 'k3_gain', 'small_frames'):
        c, st, ref = combined(emuz, name, dtype)
        for g in (1, 3):
            got = me.run_minmed(emuz, c, dtype, grid=g)
            assert all(got[k].tobytes() == ref[k].tobytes() for k in ref), (name, g)


# ---------------------------------------------------------------------------------------------------------------
# step 7
# ---------------------------------------------------------------------------------------------------------------
def seeded(lib, name, dtype):
    key = ('grow', name, np.dtype(dtype).name)
    if key not in _RUNS:
        c = mc.GROW[name]()
        med, nmed = ce.run_median(lib, c, dtype)
        frames = []
        for k in range(len(c['frames'])):
            seed, clean = ce.run_cr(lib, c, dtype, k, med, nmed)
            b = me.blot_everywhere(lib, c, dtype, k, med, nmed)[1]
            ok = ms.testable(c['frames'][k], None if c['weights'] is None else c['weights'][k],
                             None if c['masks'] is None else c['masks'][k], c['maps'][k], nmed, c['rms'][k])
            frames.append((seed, clean, b, ok))
        _RUNS[key] = (c, med, nmed, frames)
    return _RUNS[key]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', sorted(mc.GROW))
def test_grown_mask_equals_the_statement_and_clean_is_the_comparisons_blot(emuz, name, dtype):
    c, med, nmed, frames = seeded(emuz, name, dtype)
    grown_total = 0
    for k, (seed, clean0, b, ok) in enumerate(frames):
        assert seed.any(), (name, k)
        for g, cte, ctedir in c['grow']:
            mask, clean = me.run_cr_grow(emuz, c, dtype, k, med, nmed, seed, clean0, g, cte, ctedir)
            exp = ms.grow_mask(seed, ok, g, cte, ctedir)
            what = '%s frame %d g=%d c=%d dir=%d' % (name, k, g, cte, ctedir)
            assert mask.dtype == np.uint8 and np.array_equal(mask, exp.astype(np.uint8)), what
            new = exp & (seed == 0)
            assert clean[new].tobytes() == b[new].tobytes(), what      # the same b, bit for bit
            assert clean[~new].tobytes() == clean0[~new].tobytes(), what
            assert not (new & ~ok).any()
            grown_total += int(new.sum())
            if (g, cte, ctedir) == c['grow'][0]:
                for grid in (1, 3):
                    again = me.run_cr_grow(emuz, c, dtype, k, med, nmed, seed, clean0, g, cte, ctedir, grid=grid)
                    assert again[0].tobytes() == mask.tobytes() and again[1].tobytes() == clean.tobytes(), what
    assert grown_total > 0


def test_the_grow_cases_cover_what_they_claim(emuz):
    c, med, nmed, frames = seeded(emuz, 'grow_planted', np.float32)
    seed, clean0, b, ok = frames[0]
    assert {tuple(p) for p in np.argwhere(seed)} == {(j, i) for k, j, i, a in c['hits'] if k == 0}
    assert seed[7, 31] and seed[8, 32] and seed[0, 20] and seed[39, 63] and seed[39, 10]
    assert not ok[:, :3].any() and ok[:, 3:].sum() == 40 * 61 - 3           # no b in columns 0 .. 2; three masked
    g3 = ms.grow_mask(seed, ok, 3)
    assert g3[7, 30] and g3[6, 32] and g3[9, 33] and g3[1, 21] and g3[38, 62] and g3[20, 3] and g3[26, 49]
    assert not g3[25, 51] and not g3[24, 50] and not g3[10, 31]            # masked pixels inside a block: not flagged
    g9 = ms.grow_mask(seed, ok, 9)
    assert not g9[20, 2] and not g9[19, 0] and g9[24, 8] and not g9[27, 50] and g9[29, 54] and not g9[30, 55]
    down = ms.grow_mask(seed, ok, 1, 64, 1)                               # the tail runs off the frame's last row
    assert down[8:40, 31].all() and not down[6, 31] and down[39, 20] and down[9:40, 32].all()
    up = ms.grow_mask(seed, ok, 1, 5, -1)
    assert up[2:7, 31].all() and not up[1, 31] and up[3:8, 32].all() and not up[8, 31] and up[34:39, 63].all()
    assert np.array_equal(ms.grow_mask(seed, ok, 3, 64, 0), g3)            # ctedir = 0: no tail
    assert np.array_equal(ms.grow_mask(seed, ok, 1, 0, 1), seed != 0)      # g = 1, c = 0: no step 7
    c, med, nmed, frames = seeded(emuz, 'grow_dithered', np.float32)
    assert not frames[0][3][15:18, 30:34].any() and not frames[1][3][9, 40]


# ---------------------------------------------------------------------------------------------------------------
# the reason for the feature: two frames, hits in frame 0 only
# ---------------------------------------------------------------------------------------------------------------
def _visit_counts(c, masks):
    """(drawn hit pixels, those flagged in frame 0, those whose place in frame 1 is flagged as well, flagged frame-1
    pixels within 2 px of a drawn hit pixel's place)"""
    core = c['core']
    a, b = c['maps'][0], c['maps'][1]
    det = b[0] * b[4] - b[1] * b[3]
    j, i = np.nonzero(core)
    X, Y = a[0] * i + a[1] * j + a[2], a[3] * i + a[4] * j + a[5]             # frame 0 -> output -> frame 1
    x, y = (b[4] * (X - b[2]) - b[1] * (Y - b[5])) / det, (-b[3] * (X - b[2]) + b[0] * (Y - b[5])) / det
    xi, yi = np.rint(x).astype(int), np.rint(y).astype(int)
    m1 = masks[1] != 0
    place = np.zeros(m1.shape, bool)
    place[yi, xi] = True
    return int(core.sum()), int((masks[0] != 0)[core].sum()), int(m1[yi, xi].sum()), int((ms.dilate(place, 2) & m1).sum())


def test_two_frames_by_the_statement_alone():
    """'median' flags the clean frame too (the defect); 'minmed' does not, and loses no hit of frame 0"""
    c = mc.visit2()
    vals, valid = cs.singles_by_scatter(c)
    out = {}
    for how in ('median', 'minmed'):
        med, nmed, frames = ms.reject(vals, valid, c, how)
        out[how] = _visit_counts(c, [f['crmask'] for f in frames])
        print('%s: %d hit pixels drawn into frame 0, %d flagged in frame 0, %d flagged in frame 1 as well, %d flagged '
              'frame-1 pixels within 2 px of a drawn hit' % ((how,) + out[how]))
    n, med0, med_also, med_near = out['median']
    assert med_also >= 0.9 * n
    n, mm0, mm_also, mm_near = out['minmed']
    assert mm_near == 0 and mm_also == 0 and mm0 >= med0


@pytest.mark.parametrize('dtype', DTYPES)
def test_two_frames_by_the_kernels_on_cpu_threads(emuz, dtype):
    c = mc.visit2()
    out = {}
    for how in ('median', 'minmed'):
        if how == 'median':
            med, nmed = ce.run_median(emuz, c, dtype)
        else:
            got = me.run_minmed(emuz, c, dtype)
            med, nmed = got['med'], got['nmed']
        out[how] = _visit_counts(c, [ce.run_cr(emuz, c, dtype, k, med, nmed)[0] for k in range(2)])
    n, med0, med_also, med_near = out['median']
    assert med_also >= 0.9 * n
    n, mm0, mm_also, mm_near = out['minmed']
    assert mm_near == 0 and mm_also == 0 and mm0 >= med0


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
    block = header[header.index('Two or three frames'):]
    assert 'UNPINNED' in block[:block.index('2\'.')]
    table = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in ('spx_drizzle_minmed_f32', 'spx_drizzle_cr_grow_f32'):
        assert '`%s`' % name in table, name


def test_c_argument_errors_of_minmed_before_any_hip_call():
    from subpixal_amd import _ffi
    lib = _ffi.load()
    buf = np.zeros(64, np.float64)
    b = buf.ctypes.data
    nan, inf = float('nan'), float('inf')
    for fn in (lib.spx_drizzle_minmed_f32, lib.spx_drizzle_minmed_f64):
        def call(rows=b, K=2, nact=2, kernel=0, nlow=0, nhigh=0, table=b, n1=4.0, n2=3.0, grow=1, ny=4, nx=4, md=b,
                 lo=b + 8, bits=b + 16, med=b + 24, nmed=b + 32, minmed=b + 40):
            return fn(rows, K, nact, kernel, nlow, nhigh, table, n1, n2, grow, ny, nx, md, lo, bits, med, nmed, minmed,
                      None)
        for name in ('rows', 'table', 'md', 'lo', 'bits', 'med', 'nmed', 'minmed'):
            assert call(**{name: None}) == E_ARG and b'null' in lib.spx_last_error(), name
        for kw in (dict(K=0), dict(K=129), dict(K=-1), dict(nact=0), dict(nact=3), dict(nact=-1), dict(kernel=3),
                   dict(kernel=-1), dict(nlow=-1), dict(nhigh=-1), dict(n1=nan), dict(n1=inf), dict(n2=nan),
                   dict(n2=-1.0), dict(n1=2.0, n2=3.0), dict(grow=-1), dict(grow=9), dict(med=b), dict(med=b + 8),
                   dict(minmed=b + 16), dict(minmed=b + 32), dict(bits=b + 32)):
            assert call(**kw) == E_ARG, kw
            assert lib.spx_last_error()
        for kw in (dict(ny=0), dict(nx=-1), dict(ny=65536, nx=32768)):
            assert call(**kw) == E_SHAPE, kw
    assert not buf.any()


def test_c_argument_errors_of_the_growth_before_any_hip_call():
    from subpixal_amd import _ffi
    lib = _ffi.load()
    buf = np.zeros(64, np.float64)
    b = buf.ctypes.data
    for fn in (lib.spx_drizzle_cr_grow_f32, lib.spx_drizzle_cr_grow_f64):
        def call(rows=b, K=2, frame=1, fny=5, fnx=5, med=b, nmed=b, ny=8, nx=8, rms=0.1, rms_map=None, seed=b, g=3,
                 c=0, ctedir=0, crmask=b + 8, clean=b + 16):
            return fn(rows, K, frame, fny, fnx, med, nmed, ny, nx, rms, rms_map, seed, g, c, ctedir, crmask, clean, None)
        for name in ('rows', 'med', 'nmed', 'seed', 'crmask', 'clean'):
            assert call(**{name: None}) == E_ARG and b'null' in lib.spx_last_error(), name
        for kw in (dict(K=0), dict(K=129), dict(frame=-1), dict(frame=2), dict(g=0), dict(g=2), dict(g=11), dict(g=-3),
                   dict(c=-1), dict(c=65), dict(ctedir=2), dict(ctedir=-2), dict(crmask=b)):
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


OLD_KEYS = ('on', 'rms', 'gain', 'sky', 'nlow', 'nhigh', 'snr', 'scale')


def test_python_argument_errors_and_a_refused_call_changes_nothing():
    m = np.full((6, 7), 0.1, np.float32)
    nan = float('nan')
    on = dict(cr_reject=True, rms=0.1)
    for kw, what in ((dict(combine_type='mean'), 'combine_type'), (dict(combine_type=None, combine_grow=9), 'combine_grow'),
                     (dict(combine_nsigma=(3.0, 4.0)), 'combine_nsigma'), (dict(combine_nsigma=4.0), 'combine_nsigma'),
                     (dict(combine_nsigma=(4.0, nan)), 'combine_nsigma'),
                     (dict(combine_nsigma=(-1.0, -2.0)), 'combine_nsigma'),
                     (dict(combine_nsigma=(4.0, 3.0, 2.0)), 'combine_nsigma'),
                     (dict(combine_grow=-1), 'combine_grow'), (dict(combine_grow=1.5), 'combine_grow'),
                     (dict(combine_rms=[0.1, 0.1]), 'combine_rms'), (dict(combine_rms=-0.1), 'combine_rms'),
                     (dict(combine_rms=nan), 'combine_rms'), (dict(combine_rms=[0.1, m, 0.1]), 'combine_rms'),
                     (dict(driz_cr_grow=2), 'driz_cr_grow'), (dict(driz_cr_grow=11), 'driz_cr_grow'),
                     (dict(driz_cr_grow=0), 'driz_cr_grow'), (dict(driz_cr_grow=3.5), 'driz_cr_grow'),
                     (dict(driz_cr_ctegrow=-1), 'driz_cr_ctegrow'), (dict(driz_cr_ctegrow=65), 'driz_cr_ctegrow'),
                     (dict(driz_cr_ctegrow=2.5), 'driz_cr_ctegrow'),
                     (dict(driz_cr_ctedir=2), 'driz_cr_ctedir'), (dict(driz_cr_ctedir=[1, -1]), 'driz_cr_ctedir'),
                     (dict(driz_cr_ctedir=0.5), 'driz_cr_ctedir')):
        kw = {k: v for k, v in kw.items() if v is not None}
        with pytest.raises(ValueError, match=what):
            _host_drizzle(**dict(on, **kw))
        d = _host_drizzle(**on)
        before = dict(d._cr)
        with pytest.raises(ValueError, match=what):
            d.set_config_parameters(**kw)
        assert d._cr == before, kw                                  # a refused call changes nothing
    # minmed needs a scalar noise per frame: an rms MAP without combine_rms names the frame
    with pytest.raises(ValueError, match="combine_rms.*'b'"):
        _host_drizzle(cr_reject=True, rms=[0.1, m, 0.1], combine_type='minmed')
    d = _host_drizzle(cr_reject=True, rms=[0.1, m, 0.1])
    before = dict(d._cr)
    with pytest.raises(ValueError, match="combine_rms.*'b'"):
        d.set_config_parameters(combine_type='minmed')
    assert d._cr == before and d._cr['combine'] == 'median'
    d.set_config_parameters(combine_type='minmed', combine_rms=[0.1, 0.2, 0.3], combine_nsigma=(5, 2), combine_grow=0,
                            driz_cr_grow=3, driz_cr_ctegrow=7, driz_cr_ctedir=[1, 0, -1])
    assert d._cr['combine'] == 'minmed' and d._cr['combine_rms'] == dict(a=0.1, b=0.2, c=0.3)
    assert d._cr['nsigma'] == (5.0, 2.0) and d._cr['combine_grow'] == 0 and d._cr['grow'] == 3
    assert d._cr['ctegrow'] == 7 and d._cr['ctedir'] == dict(a=1, b=0, c=-1)
    # with the feature off the new keywords are accepted and unused
    q = _host_drizzle(combine_type='minmed', driz_cr_grow=5)
    assert q.output_minmed is None and q.crseed('a') is None and q.output_crclean is None


def test_defaults_leave_the_existing_configuration_and_the_call_sequence_as_they_are():
    from subpixal_amd import resample
    d = _host_drizzle(cr_reject=True, rms=0.1)
    assert {k: d._cr[k] for k in OLD_KEYS} == dict(on=True, rms=dict(a=0.1, b=0.1, c=0.1), gain=None, sky=None, nlow=0,
                                                   nhigh=0, snr=(3.5, 3.0), scale=(1.2, 0.7))
    assert d._cr['combine'] == 'median' and d._cr['grow'] == 1 and d._cr['ctegrow'] == 0
    assert d._cr['nsigma'] == (4.0, 3.0) and d._cr['combine_grow'] == 1 and d._cr['combine_rms'] is None
    assert d.output_minmed is None and d.crseed('a') is None
    sig = inspect.signature(resample.DeviceDrizzle.__init__).parameters
    for key, default in (('combine_type', 'median'), ('combine_nsigma', (4.0, 3.0)), ('combine_grow', 1),
                         ('combine_rms', None), ('driz_cr_grow', 1), ('driz_cr_ctegrow', 0), ('driz_cr_ctedir', 0)):
        assert sig[key].default == default, key
        assert key in inspect.signature(resample.DeviceDrizzle.set_config_parameters).parameters
    # which entries a configuration calls: the defaults call what they called, the new entries only when asked for
    assert d._cr_entries() == ('spx_drizzle_median', 'spx_drizzle_cr')
    assert _host_drizzle(cr_reject=True, rms=0.1, driz_cr_grow=1, driz_cr_ctegrow=9, driz_cr_ctedir=0)._cr_entries() == \
        ('spx_drizzle_median', 'spx_drizzle_cr')
    assert _host_drizzle(cr_reject=True, rms=0.1, combine_type='minmed')._cr_entries() == \
        ('spx_drizzle_minmed', 'spx_drizzle_cr')
    assert _host_drizzle(cr_reject=True, rms=0.1, driz_cr_grow=3)._cr_entries() == \
        ('spx_drizzle_median', 'spx_drizzle_cr', 'spx_drizzle_cr_grow')
    assert _host_drizzle(cr_reject=True, rms=0.1, driz_cr_ctegrow=4, driz_cr_ctedir=[0, 1, 0])._cr_entries() == \
        ('spx_drizzle_median', 'spx_drizzle_cr', 'spx_drizzle_cr_grow')
