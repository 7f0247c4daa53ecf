"""Whole-frame sigma-clipped statistics without a GPU: the kernels of subpixal_amd/csrc/spx_sky_kernels.h on CPU
threads (tests/cpu_emu/emu_sky.cpp, the library's own launch sequence) against the numpy statement of
tests/sky_statement.py on every case of tests/sky_cases.py: counts, rounds, status and the median exactly, the edges
and the moments within the statement's bounds, `sky` by the rule; every case is SAFE by the statement alone (cap 0);
batch position, a second run and the hist kernel's grid do not change a bit; the mesh family agrees on a 64 x 64
cell; every argument check of the new C entries; the ValueErrors and the bookkeeping of `resample.DeviceDrizzle`'s
sky subtraction on the host."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import sky_cases as sc
import sky_emu as se
import sky_statement as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('spx_sky_workspace_bytes', 'spx_sky_stats_f32', 'spx_sky_stats_f64')
E_ARG, E_WORKSPACE = -1, -4
CASES = [(n, dt) for n in sorted(sc.ALL) for dt in sc.dtypes(n)]
IDS = ['%s-%s' % (n, dt.name) for n, dt in CASES]


@pytest.fixture(scope='module')
def emus(tmp_path_factory):
    return se.load(tmp_path_factory)


# ---------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,dtype', CASES, ids=IDS)
def test_case_against_the_statement(emus, name, dtype):
    c = sc.ALL[name](dtype)
    st = se.statements(name, c, dtype)
    got, _ = se.run(emus, c, dtype)
    assert len(got) == len(st)
    for k, (g, s) in enumerate(zip(got, st)):
        ss.check(g, s, c['stat'], '%s %s frame %d' % (name, dtype.name, k))


@pytest.mark.parametrize('name,dtype', CASES, ids=IDS)
def test_the_statement_alone_finds_every_case_safe(name, dtype):
    """no kernel anywhere: in every round of every frame the nearest usable value is farther from each new edge than
    the bound on that edge, and std exceeds its bound.  The cap on unsafe cases is zero."""
    st = se.statements(name, sc.ALL[name](dtype), dtype)
    for k, s in enumerate(st):
        assert s['safe'], (name, k, s['margins'])


@pytest.mark.parametrize('name,dtype', CASES, ids=IDS)
def test_every_case_covers_what_it_names(name, dtype):
    c = sc.ALL[name](dtype)
    assert all(f.shape[0] <= 61 and f.shape[1] <= 101 for f in c['frames'])
    assert sc.COVERS[name](se.statements(name, c, dtype)), name


def test_the_case_list_covers_the_dtypes_and_the_stats():
    assert {dt.name for _, dt in CASES} == {'float32', 'float64'}
    assert {sc.ALL[n](dt)['stat'] for n, dt in CASES} == {'median', 'mean', 'mode'}
    assert any(sc.ALL[n](dt)['lsigma'] != sc.ALL[n](dt)['usigma'] for n, dt in CASES)


# ---------------------------------------------------------------------------------------------------------------
# reproducibility
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.dtype(np.float32), np.dtype(np.float64)], ids=['float32', 'float64'])
def test_alone_or_in_a_batch_same_bits(emus, dtype):
    c = sc.ALL['batch_of_five'](dtype)
    rows, _ = se.run(emus, c, dtype)
    for k in (0, 1, 2, 4):
        alone, _ = se.run(emus, c, dtype, frames_only=[k])
        a, b = alone[0], rows[k]
        assert sorted(a) == sorted(b)
        for key in a:
            assert np.array([a[key]]).tobytes() == np.array([b[key]]).tobytes(), (k, key, a[key], b[key])


@pytest.mark.parametrize('name,dtype', [('asymmetric_factors', np.dtype(np.float32)),
                                        ('thread_takes_two_pixels', np.dtype(np.float64))])
def test_second_run_and_another_hist_grid_same_bits(emus, name, dtype):
    c = sc.ALL[name](dtype)
    _, first = se.run(emus, c, dtype, gpf=1)
    _, second = se.run(emus, c, dtype, gpf=1)
    _, other = se.run(emus, c, dtype, gpf=3)
    assert first == second == other


def test_frame_reads_counted_from_the_launch_sequence(emus):
    # (max_iters + 1) (D + 1): 24 reads of a float32 frame and 42 of a float64 frame at the default clip = 5
    assert emus.emus_sky_frame_reads(3, 5) == 24 and emus.emus_sky_frame_reads(6, 5) == 42
    assert emus.emus_sky_frame_reads(3, 0) == 4


# ---------------------------------------------------------------------------------------------------------------
# the mesh family on one 64 x 64 cell
# ---------------------------------------------------------------------------------------------------------------
def test_cross_check_with_the_background_mesh(emus, tmp_path_factory):
    """spx_background_mesh_f32 with ONE 64 x 64 cell (through its own harness, emu_background.cpp) and the whole-frame
    statistics with lsigma = usigma = kappa follow the same rule: n and med are equal; mean and std agree within the
    sum of the two bounds.  The mesh's sums are over 4096 values in chains of 16 + 16 + 16 additions, its mean is
    sum / m and its std the two-pass form about that mean: |d mean| <= 50 u mean|v|, |d std| <= 52 u std + |d mean|,
    doubled as the statement's bounds are."""
    so = str(tmp_path_factory.mktemp('emub') / 'libspx_emu_background.so')
    subprocess.check_call(se.emu_flags() + ['-shared', '-o', so,
                                            os.path.join(ROOT, 'tests', 'cpu_emu', 'emu_background.cpp')])
    lib = ctypes.CDLL(so)
    kappa, iters = 2.5, 3
    frame = sc.with_sources(sc.noise(31, 64, 64, np.float32), 32, 6, 300.0)
    mb, mr, ng = np.zeros((1, 1)), np.zeros((1, 1)), np.zeros((1, 1), np.int32)
    trace = np.zeros((1, 1, 5))
    assert lib.emub_mesh_f32(se._p(frame), None, None, 64, 64, 64, 64, ctypes.c_double(kappa), iters,
                             ctypes.c_double(0.0), se._p(mb), se._p(mr), se._p(ng), se._p(trace), 1) == 0
    c = sc.make([frame], lsigma=kappa, usigma=kappa, max_iters=iters, stat='mode')
    st = ss.statement(frame, lsigma=kappa, usigma=kappa, max_iters=iters, stat='mode')
    assert st['safe'] and st['rounds'] >= 2, st['margins']
    got = se.run(emus, c, np.float32)[0][0]
    ss.check(got, st, 'mode', 'mesh cross-check')
    lo, hi, med, mean, std = trace[0, 0]
    assert int(ng[0, 0]) == got['n_usable'] == 4096
    assert int(hi - lo) == got['n_final'] < 4096
    assert med == got['med']
    b_mean = 2 * 50 * ss.U * float(np.abs(frame).mean())
    b_std = 2 * (52 * ss.U * std + b_mean)
    assert abs(mean - got['mean']) <= st['b_mean'] + b_mean
    assert abs(std - got['std']) <= st['b_std'] + b_std
    assert abs(mb[0, 0] - got['sky']) <= 4 * (st['b_mean'] + b_mean)      # the same 'mode' rule on both


# ---------------------------------------------------------------------------------------------------------------
# the C entries' argument checks (all made before any HIP call: no device needed)
# ---------------------------------------------------------------------------------------------------------------
def _call(lib, **kw):
    a = dict(frames=8, weights=None, masks=None, shapes=8, K=2, lower=float('nan'), upper=float('nan'), lsigma=4.0,
             usigma=4.0, iters=5, stat=0, work=8, work_bytes=lib.spx_sky_workspace_bytes(2), out=8, counts=8, status=8,
             fn=lib.spx_sky_stats_f32)
    a.update(kw)
    return a['fn'](a['frames'], a['weights'], a['masks'], a['shapes'], a['K'], a['lower'], a['upper'], a['lsigma'],
                   a['usigma'], a['iters'], a['stat'], a['work'], a['work_bytes'], a['out'], a['counts'], a['status'],
                   None)


def test_argument_checks_of_the_new_entries():
    from subpixal_amd import _ffi
    lib = _ffi.load()
    assert lib.spx_sky_workspace_bytes(0) == 0 and lib.spx_sky_workspace_bytes(129) == 0
    assert lib.spx_sky_workspace_bytes(-1) == 0
    one = lib.spx_sky_workspace_bytes(1)
    assert one > 0 and lib.spx_sky_workspace_bytes(128) == 128 * one
    for fn in (lib.spx_sky_stats_f32, lib.spx_sky_stats_f64):
        for name in ('frames', 'shapes', 'out', 'counts', 'status'):
            assert _call(lib, fn=fn, **{name: None}) == E_ARG and b'null' in lib.spx_last_error(), name
        inf, nan = float('inf'), float('nan')
        for kw in (dict(K=0), dict(K=129), dict(K=-3), dict(lsigma=0.0), dict(lsigma=-1.0), dict(lsigma=inf),
                   dict(lsigma=nan), dict(usigma=0.0), dict(usigma=inf), dict(usigma=nan), dict(iters=-1),
                   dict(stat=3), dict(stat=-1), dict(lower=2.0, upper=1.0)):
            assert _call(lib, fn=fn, **kw) == E_ARG, kw
        assert _call(lib, fn=fn, work=None) == E_WORKSPACE
        assert _call(lib, fn=fn, work_bytes=lib.spx_sky_workspace_bytes(2) - 1) == E_WORKSPACE
        assert _call(lib, fn=fn, work_bytes=0) == E_WORKSPACE


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
    for k, v in _ffi.SKY_STATS.items():
        assert '#define SPX_SKY_%s %d' % (k.upper(), v) in header
    assert '#define SPX_SKY_EMPTY %d' % _ffi.SKY_EMPTY in header
    assert '#define SPX_SKY_BAD_FRAME %d' % _ffi.SKY_BAD_FRAME in header
    table = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW:
        assert '`%s`' % name in table, name


def test_no_existing_kernel_header_includes_the_new_one():
    csrc = os.path.join(ROOT, 'subpixal_amd', 'csrc')
    for fn in os.listdir(csrc):
        if fn.endswith('.h') and fn != 'spx_sky_kernels.h':
            assert 'spx_sky_kernels.h' not in open(os.path.join(csrc, fn)).read(), fn


# ---------------------------------------------------------------------------------------------------------------
# sky.frame_stats and resample.DeviceDrizzle on the host, before the device is touched
# ---------------------------------------------------------------------------------------------------------------
def test_frame_stats_value_errors():
    from subpixal_amd import sky
    f = np.zeros((5, 7), np.float32)
    for kw in (dict(stat='mod'), dict(lower=2.0, upper=1.0), dict(clip=-1), dict(clip=1.5), dict(lsigma=0.0),
               dict(usigma=float('inf')), dict(lsigma=float('nan'))):
        with pytest.raises(ValueError):
            sky.frame_stats([f], **kw)
    for frames, kw in (([], {}), ([f] * 129, {}), ([f.astype(np.int32)], {}), ([f, f.astype(np.float64)], {}),
                       ([f[0]], {}), ([f], dict(weights=[f[:3]])), ([f], dict(masks=[f[:, :2]])),
                       ([f], dict(weights=[f, f]))):
        with pytest.raises(ValueError):
            sky.frame_stats(frames, **kw)


def _host_drizzle(K=3, **kw):
    from subpixal_amd import resample
    names = ['a', 'b', 'c', 'd'][:K]
    frames = [np.zeros((12, 14), np.float32) for _ in range(K)]
    maps = [[1.0, 0.0, float(k), 0.0, 1.0, 0.0] for k in range(K)]
    return resample.DeviceDrizzle(frames, maps, (16, 20), names=names, **kw)


def test_drizzle_sky_keywords_and_value_errors():
    d = _host_drizzle()
    assert d._skycfg['on'] is False and d.computed_sky == {} and not d._sub
    d = _host_drizzle(skysub=True, skystat='mode', skymethod='globalmin', skylower=-5.0, skyupper=900.0, skyclip=3,
                      skylsigma=2.5, skyusigma=3.0)
    assert d._skycfg == dict(on=True, stat='mode', method='globalmin', lower=-5.0, upper=900.0, clip=3, lsigma=2.5,
                             usigma=3.0, user=None)
    for kw in (dict(skystat='mod'), dict(skymethod='match'), dict(skylower=2.0, skyupper=1.0), dict(skyclip=-1),
               dict(skylsigma=0.0), dict(skyusigma=float('nan')), dict(skyuser=[1.0, 2.0]),
               dict(skyuser=[1.0, 2.0, float('nan')]), dict(skyuser=[1.0, 2.0, np.zeros((12, 14))])):
        with pytest.raises(ValueError):
            _host_drizzle(skysub=True, **kw)
        d = _host_drizzle(skysub=True)
        before = dict(d._skycfg)
        with pytest.raises(ValueError):
            d.set_config_parameters(**kw)
        assert d._skycfg == before                                  # a refused call changes nothing
    # sky= belongs to the unsubtracted comparison
    with pytest.raises(ValueError, match='skysub'):
        _host_drizzle(skysub=True, sky=3.0, cr_reject=True, rms=1.0)
    with pytest.raises(ValueError, match='skysub'):
        _host_drizzle(skysub=True, sky=[1.0, 2.0, 3.0])
    d = _host_drizzle(sky=3.0)
    with pytest.raises(ValueError, match='skysub'):
        d.set_config_parameters(skysub=True)
    d = _host_drizzle(skysub=True)
    with pytest.raises(ValueError, match='skysub'):
        d.set_config_parameters(sky=1.0)
    # cr_reject with a PolyMap stays the error it is, with or without skysub
    from subpixal_amd.resample import PolyMap
    d = _host_drizzle(skysub=True, cr_reject=True, rms=1.0)
    with pytest.raises(ValueError, match='polynomial'):
        d.set_map('a', PolyMap.from_affine([1, 0, 0, 0, 1, 0]))
    d = _host_drizzle(skysub=True)
    d.set_map('a', PolyMap.from_affine([1, 0, 0, 0, 1, 0]))          # skysub never looks at the maps


def test_drizzle_sky_freezing_and_copy():
    d = _host_drizzle(skysub=True, skyuser=[1.0, 2.0, 3.0])
    assert d.computed_sky == {}                                     # nothing exists before the first execute()
    d._sky = dict(a=1.0, b=2.0, c=3.0)                              # as the first execute() leaves them
    d._sub = dict(a=(1.0, 'ta'), b=(2.0, 'tb'), c=(3.0, 'tc'))
    got = d.computed_sky
    got['a'] = 99.0
    assert d.computed_sky == dict(a=1.0, b=2.0, c=3.0)              # a copy is handed out
    # keywords that are not sky keywords keep the values frozen
    d.set_config_parameters(pixfrac=0.8, fill=1.0)
    d.set_config_parameters(skyclip=5, skystat='median')            # the values they have already: nothing changes
    assert d.computed_sky == dict(a=1.0, b=2.0, c=3.0) and len(d._sub) == 3
    # a copy shares tensors and values, in dicts of its own
    q = d.copy()
    assert q.computed_sky == d.computed_sky and q._sky is not d._sky and q._sub is not d._sub
    assert q._sub['b'][1] is d._sub['b'][1] and q._skycfg == d._skycfg and q._skycfg is not d._skycfg
    q.computed_sky = dict(a=5.0)
    assert q.computed_sky == dict(a=5.0) and not q._sub and q._stale
    assert d.computed_sky == dict(a=1.0, b=2.0, c=3.0) and len(d._sub) == 3
    for bad in (dict(z=1.0), dict(a=float('nan')), dict(a=np.zeros(2))):
        with pytest.raises(ValueError):
            q.computed_sky = bad
        assert q.computed_sky == dict(a=5.0)
    # changing a sky keyword unfreezes
    d.set_config_parameters(skylsigma=3.0)
    assert d.computed_sky == {} and not d._sub and d._stale
    d._sky = dict(a=1.0)
    d.set_config_parameters(skysub=False)
    assert d.computed_sky == {} and d._skycfg['on'] is False
    # off: the rows point at the frames as given, whatever is stored
    d._sub = dict(a=(1.0, 'ta'))
    assert d._sci('a') is d._pool['a'].data


def test_drizzle_packs_the_subtracted_tensor(monkeypatch):
    """with skysub the row of a frame carries the pointer of its subtracted tensor, without it the frame's own; a
    dropped frame without a value keeps its own (the kernel skips its row)"""
    class T(object):
        def __init__(self, p, shape=(12, 14)):
            self.p, self.shape = p, shape

        def data_ptr(self):
            return self.p
    d = _host_drizzle(skysub=True, skyuser=[1.0, 2.0, 3.0])
    for k, n in enumerate('abc'):
        d._pool[n].data, d._pool[n].resident = T(1000 + 16 * k), True
    d._sky = dict(a=1.0, b=2.0)
    d._sub = dict(a=(1.0, T(5000)), b=(2.0, T(5016)))
    d._active['c'] = False
    rows = d._pack(['a', 'b', 'c'])
    assert [int(r[:8].view(np.uint64)[0]) for r in rows] == [5000, 5016, 1032]
    d.set_config_parameters(skysub=False)
    rows = d._pack(['a', 'b', 'c'])
    assert [int(r[:8].view(np.uint64)[0]) for r in rows] == [1000, 1016, 1032]
