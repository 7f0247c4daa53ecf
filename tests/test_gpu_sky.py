"""Whole-frame sky statistics and the drizzle's sky subtraction on the device.

(a) Every case of tests/sky_cases.py through `sky.frame_stats` (spx_sky_stats_*): against the numpy statement of
    tests/sky_statement.py as tests/test_sky_cpu.py does, and bit-identical to the same kernel source run on CPU
    threads (tests/cpu_emu/emu_sky.cpp).
(b) `DeviceDrizzle(skysub=True)` on a 96 x 96, K = 3 scene with pedestals and one `PolyMap` frame: `computed_sky`
    is `sky.frame_stats`'s; the outputs are bit-identical to a drizzle of frames subtracted beforehand with the same
    float32 subtraction, also after `fast_replace_image(drop=...)` and in a `copy()`, and neither moves the values;
    the same for 'globalmin' and `skyuser`; with `skysub=False` nothing differs from a call without the keywords.
(c) Equivariance: sky(frame + p) - sky(frame) = p on frame 0 of the scene of (d).
(d) End to end on the scene of tests/test_gpu_crreject.py (384 x 384, 81 sources, K = 4, 150 drawn hits per frame,
    frame 3 off by 0.3 px) with pedestals of (0, 5, 10, 20) x the noise sigma added to the four frames.  Three runs:
      1. no pedestals, cr_reject=True: today's path, the yardstick;
      2. pedestals, cr_reject=True, skysub=True: the flagged share of frames 0 .. 2 stays under the drawn share plus
         0.5 %, the offset within the standing 2e-4 px of the yardstick, the matrix within the allowance of
         test_gpu_crreject.py -- 3 sqrt(2) sigma / (sqrt(N) L), the same formula, from the YARDSTICK's own per-source
         scatter sigma, its N kept sources and their lever arm L, and nothing of the run under test;
      3. pedestals, cr_reject=True, no skysub: frame 3 lies 12.5 sigma above its blot, so more than half of it must
         come out flagged.  This is the evidence that the feature is needed.
    The sky errors `computed - drawn` carry the sources' bias (the wings of 81 sources lift the median); they are
    printed and not bounded in advance.

    Measured on an MI355X (offset error px / matrix error; DESIGN.md section 7 has the same):
        1. no pedestals, cr_reject            1.066e-3 / 3.967e-6   (81 sources); flagged 0.2109 0.2102 0.2143 0.2211 %
        2. pedestals, cr_reject, skysub       1.067e-3 / 3.967e-6   (81 sources); flagged 0.2109 0.2102 0.2143 0.2211 %
        3. pedestals, cr_reject, no skysub    frame 3 flagged to 89.77 % (frames 0 .. 2: 87.59 %, 1.95 %, 0.53 %)
        drawn hit pixels 0.2082 % of frames 0 .. 2; yardstick sigma 1.462e-3 px, N = 74, L = 91.6 px: allowance 7.875e-6
        sky errors computed - drawn, in units of the noise: +0.0908 +0.0913 +0.0907 +0.0862
    (c) measured: sky(frame + p) - sky(frame) - p = 1.2e-9 against the derived bound 7.1e-7 (h = 1.2e-7).
"""
import os
import sys

import numpy as np
import pytest

import sky_cases as sc
import sky_emu as se
import sky_statement as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

pytestmark = pytest.mark.gpu
CASES = [(n, dt) for n in sorted(sc.ALL) for dt in sc.dtypes(n)]
IDS = ['%s-%s' % (n, dt.name) for n, dt in CASES]
_DEVICE, _EMU = {}, {}


def device_rows(name, dtype):
    """a case on the device, run once and shared (read-only): per frame a dict of results"""
    from subpixal_amd import sky
    key = (name, dtype.name)
    if key not in _DEVICE:
        c = sc.ALL[name](dtype)
        frames, weights, masks, K = se.prepared(c, dtype)
        r = sky.frame_stats(frames, weights, masks, stat=c['stat'], lower=c['lower'], upper=c['upper'],
                            clip=c['max_iters'], lsigma=c['lsigma'], usigma=c['usigma'])
        _DEVICE[key] = c, [dict(sky=r.sky[k], med=r.median[k], mean=r.mean[k], std=r.std[k], lo=r.lo[k], hi=r.hi[k],
                                n_usable=r.n_usable[k], n_final=r.n_final[k], rounds=r.rounds[k], status=r.status[k])
                           for k in range(K)]
    return _DEVICE[key]


# ---------------------------------------------------------------------------------------------------------------
# (a)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,dtype', CASES, ids=IDS)
def test_case_against_the_statement(name, dtype):
    c, rows = device_rows(name, dtype)
    st = se.statements(name, c, dtype)
    assert len(rows) == len(st)
    for k, (g, s) in enumerate(zip(rows, st)):
        ss.check({key: (float(v) if key in se.COLUMNS else int(v)) for key, v in g.items()}, s, c['stat'],
                 '%s %s frame %d' % (name, dtype.name, k))


@pytest.mark.parametrize('name,dtype', CASES, ids=IDS)
def test_bit_identical_to_the_kernels_on_cpu_threads(tmp_path_factory, name, dtype):
    emus = se.load(tmp_path_factory)
    c, rows = device_rows(name, dtype)
    erows, _ = se.run(emus, c, dtype, gpf=1)
    for k, (g, e) in enumerate(zip(rows, erows)):
        for key in se.COLUMNS:
            assert np.float64(g[key]).tobytes() == np.float64(e[key]).tobytes(), (name, k, key, g[key], e[key])
        for key in ('n_usable', 'n_final', 'rounds', 'status'):
            assert int(g[key]) == e[key], (name, k, key)


def test_tensors_on_the_device_and_a_second_call_same_bits():
    import torch
    from subpixal_amd import sky
    c = sc.ALL['batch_of_five'](np.dtype(np.float32))
    frames, weights, masks, K = se.prepared(c, np.float32)
    kw = dict(stat=c['stat'], clip=c['max_iters'], lsigma=c['lsigma'], usigma=c['usigma'])
    a = sky.frame_stats(frames, weights, masks, **kw)
    b = sky.frame_stats([torch.from_numpy(f).cuda() for f in frames],
                        [None if w is None else torch.from_numpy(w).cuda() for w in weights],
                        [None if m is None else torch.from_numpy(m).cuda() for m in masks], **kw)
    for col in sky.SkyStats.__slots__:
        assert getattr(a, col).tobytes() == getattr(b, col).tobytes(), col
    assert a.status.tolist() == [0, sky.EMPTY, 0, 0, 0] and len(a) == 5


# ---------------------------------------------------------------------------------------------------------------
# (b)
# ---------------------------------------------------------------------------------------------------------------
def _bytes(d):
    return tuple(t.cpu().numpy().tobytes() for t in (d.output_sci, d.output_wht, d.output_ctx))


def test_device_drizzle_with_skysub():
    import bench_drizzle as bd
    from subpixal_amd import resample, sky
    N, K = 96, 3
    s = bd.dither_scene(N, 9, K, seed=3, sigma=2.5, border=20.0)
    ped = [np.float32(p * s['noise']) for p in (7.0, 0.0, 15.0)]
    frames = [f + p for f, p in zip(s['frames'], ped)]
    assert all(f.dtype == np.float32 for f in frames)
    c = 0.5 * (N - 1)
    poly = resample.PolyMap.from_affine(s['truth'][2], center=(c, c))
    coef = poly.coef.copy()
    coef[0, 3], coef[1, 5] = 2e-5, -1.5e-5                          # a little distortion: u^2 in X, v^2 in Y
    maps = [s['truth'][0], s['truth'][1], resample.PolyMap(coef, 2, (c, c))]
    mask0 = np.zeros((N, N), np.uint8)
    mask0[40:44, 10:30] = 1
    w1 = np.ones((N, N), np.float32)
    w1[:, :5] = 0.0
    masks, weights = [mask0, None, None], [None, w1, None]
    kw = dict(masks=masks, weights=weights)
    d = resample.DeviceDrizzle(frames, maps, (N, N), skysub=True, **kw)
    assert d.computed_sky == {} and not d._sub
    d.execute()
    st = sky.frame_stats(frames, weights, masks)
    got = d.computed_sky
    assert sorted(got) == [0, 1, 2] and [got[k] for k in range(K)] == st.sky.tolist()
    print('computed - drawn sky, in units of the noise:', [(got[k] - float(ped[k])) / s['noise'] for k in range(K)])
    assert all(abs(got[k] - float(ped[k])) < s['noise'] for k in range(K))

    def subtracted(values):
        return [f - np.float32(v) for f, v in zip(frames, values)]
    ref = resample.DeviceDrizzle(subtracted(st.sky), maps, (N, N), **kw).execute()
    assert _bytes(d) == _bytes(ref)
    assert d.science(1).cpu().numpy().tobytes() == subtracted(st.sky)[1].tobytes()
    assert d._pool[1].data.cpu().numpy().tobytes() == frames[1].tobytes()       # the frame as given is kept
    # a copy and a fast replace: the same outputs as on the subtracted frames, and the values stay
    q = d.copy()
    q.fast_replace_image(drop=1)
    ref.fast_replace_image(drop=1)
    assert _bytes(q) == _bytes(ref) and _bytes(q) != _bytes(d)
    assert q.computed_sky == got and d.computed_sky == got and q.science(0) is d.science(0)
    q.fast_add_image(1)
    ref.fast_add_image(1)
    assert _bytes(q) == _bytes(ref) and q.computed_sky == got
    # a second full execute() reuses the frozen values: no new tensor
    before = d.science(2)
    d.execute()
    assert d.science(2) is before and _bytes(d) == _bytes(resample.DeviceDrizzle(subtracted(st.sky), maps, (N, N),
                                                                                   **kw).execute())
    # globalmin, skyuser, an assigned computed_sky
    g = resample.DeviceDrizzle(frames, maps, (N, N), skysub=True, skymethod='globalmin', **kw).execute()
    low = float(st.sky.min())
    assert g.computed_sky == {0: low, 1: low, 2: low}
    assert _bytes(g) == _bytes(resample.DeviceDrizzle(subtracted(K * [low]), maps, (N, N), **kw).execute())
    user = [0.25, -0.5, 1.0]
    u = resample.DeviceDrizzle(frames, maps, (N, N), skysub=True, skyuser=user, **kw).execute()
    assert u.computed_sky == dict(enumerate(user))
    assert _bytes(u) == _bytes(resample.DeviceDrizzle(subtracted(user), maps, (N, N), **kw).execute())
    u.computed_sky = {1: 0.75}
    u.execute()
    assert u.computed_sky == {0: 0.25, 1: 0.75, 2: 1.0}
    assert _bytes(u) == _bytes(resample.DeviceDrizzle(subtracted([0.25, 0.75, 1.0]), maps, (N, N), **kw).execute())
    # another statistic unfreezes
    d.set_config_parameters(skystat='mode', skyclip=3, skylsigma=3.0, skyusigma=3.0)
    assert d.computed_sky == {}
    d.execute()
    mode = sky.frame_stats(frames, weights, masks, stat='mode', clip=3, lsigma=3.0, usigma=3.0)
    assert [d.computed_sky[k] for k in range(K)] == mode.sky.tolist() and mode.sky.tolist() != st.sky.tolist()
    # off: today's call, bit for bit, and nothing of the feature is there
    off = resample.DeviceDrizzle(frames, maps, (N, N), skysub=False, **kw).execute()
    today = resample.DeviceDrizzle(frames, maps, (N, N), **kw).execute()
    assert _bytes(off) == _bytes(today) and _bytes(off) != _bytes(d)
    assert off.computed_sky == {} and not off._sub and off.science(0) is off._pool[0].data
    # the same row bytes: behind the three pointers (data, weight, mask) of each row nothing differs
    assert off._rows_host.shape == today._rows_host.shape
    assert off._rows_host[:, 24:].tobytes() == today._rows_host[:, 24:].tobytes()


# ---------------------------------------------------------------------------------------------------------------
# (c)
# ---------------------------------------------------------------------------------------------------------------
CROSSERS = 12


def test_sky_is_equivariant_under_a_pedestal():
    """sky(frame + p) - sky(frame) = p for the median of frame 0 of the scene of (d), p = 20 x the noise, within a
    bound made of two parts, both fixed before the run:
      * v -> fl32(v + p) is monotone, so the order statistics of an unchanged set keep their ranks and each moves by
        p up to one rounding: h = half an ulp of float32 at the largest |v + p| of the frame;
      * the sets can differ.  Every value is off by at most h, so the median by at most h and std by at most 2 h
        against the shifted originals; an edge med -+ 4 std therefore moves by at most 9 h against the data and only
        values within 10 h of an edge can change sides.  At 4 std the frame's density is n phi(4) / std per unit, so
        per edge and round n phi(4) 10 h / std = 147456 x 1.3e-4 x 10 h / std values are expected to cross: with
        h = 1.2e-7 (values up to 2.04) and std = 0.002 that is 0.012, and twelve rounds-times-edges make 0.14 in all
        (sources' wings raise the density at the upper edge a few times).  The test allows CROSSERS =
        12 (one per edge and round of the six rounds), each of which moves the median's rank by half a step: the
        median may move by the distance between the order statistics 12 ranks either side of it, read off the
        sorted ORIGINAL frame on the host.
    bound = h + (s[k + 12] - s[k - 12]), k the rank of the median among the sorted pixels of the frame."""
    import test_gpu_drizzle_align as ta
    from subpixal_amd import sky
    s = ta.scene()
    frame = s['frames'][0]
    p = np.float32(20.0 * s['noise'])
    shifted = frame + p
    assert shifted.dtype == np.float32
    r = sky.frame_stats([frame, shifted])
    h = 0.5 * float(np.spacing(np.float32(np.abs(shifted).max())))
    srt = np.sort(frame.ravel().astype(np.float64))
    k = int(np.searchsorted(srt, r.median[0]))
    bound = h + float(srt[k + CROSSERS] - srt[k - CROSSERS])
    err = abs((r.sky[1] - r.sky[0]) - float(p))
    print('sky %.9g -> %.9g, p = %.9g: off by %.3e, bound %.3e (h = %.3e), n_final %d and %d, rounds %d and %d'
          % (r.sky[0], r.sky[1], float(p), err, bound, h, r.n_final[0], r.n_final[1], r.rounds[0], r.rounds[1]))
    assert r.rounds[0] >= 2 and r.status.tolist() == [0, 0]
    assert err <= bound
    assert bound < 1e-2 * s['noise']                         # the bound says something: a hundredth of the noise


# ---------------------------------------------------------------------------------------------------------------
# (d)
# ---------------------------------------------------------------------------------------------------------------
PEDESTALS = (0.0, 5.0, 10.0, 20.0)
_RUNS = {}


def three_runs():
    import test_gpu_crreject as tc
    import test_gpu_drizzle_align as ta
    from subpixal_amd import align, resample
    if 'r' in _RUNS:
        return _RUNS['r']
    s = ta.scene()
    SIZE = ta.SIZE
    maps = [m.copy() for m in s['truth']]
    maps[3] = ta.perturbed(s['truth'], 3)
    hit_frames, drawn = tc.add_hits(s['frames'], np.random.default_rng(41), tc.HITS, 0.3, 3.0)
    ped = [np.float32(p * s['noise']) for p in PEDESTALS]
    ped_frames = [f + p for f, p in zip(hit_frames, ped)]
    npix = sum(len(h) for h in drawn[:3])
    out = dict(drawn=npix / (3.0 * SIZE * SIZE))
    for what, frames, kw in (('yardstick', hit_frames, {}), ('skysub', ped_frames, dict(skysub=True)),
                             ('no skysub', ped_frames, {})):
        drz = resample.DeviceDrizzle(frames, np.stack(maps), (SIZE, SIZE), cr_reject=True, rms=s['noise'], **kw)
        drz.execute()
        flagged = [float(drz.crmask(k).sum()) / (SIZE * SIZE) for k in range(4)]
        out[what + ' flagged'] = flagged
        print('%s: flagged share per frame %s' % (what, ' '.join('%.4f %%' % (100 * f) for f in flagged)))
        if what == 'no skysub':
            break                                             # frame 3 is gone: there is nothing to fit
        if kw:
            sk = drz.computed_sky
            out['sky errors'] = [(sk[k] - float(ped[k])) / s['noise'] for k in range(4)]
            print('computed - drawn sky in units of the noise: %s' % ' '.join('%+.4f' % e for e in out['sky errors']))
        q = drz.copy()
        q.fast_drop_image(3)
        cat = ta.catalog()
        cat.set_image(q.output_sci)
        cat.execute()
        prim = cat.cutout_catalog(q.output_sci, pad=1, weight='pos_std')
        img_cat, drz_cat, aff = align._frame_catalogs(q, 3, prim, 6, np.float32)
        fit, _, _ = align.find_linear_fit(img_cat, drz_cat, affine=aff, fitgeom='general', nclip=3, sigma=3.0)
        out[what] = ta.errors(align.compose_fit(maps[3], fit), s['truth'][3]) + (len(img_cat),)
        if what == 'yardstick':
            keep = np.asarray(fit['fitmask'], bool)
            pos = np.asarray(img_cat.src_pos, np.float64)[keep]
            sigma, n = float(np.max(fit['rms'])), int(keep.sum())
            lever = float(np.sqrt(np.mean(np.var(pos, axis=0))))
            out['allowance'] = 3.0 * np.sqrt(2.0) * sigma / (np.sqrt(n) * lever)
            print('yardstick fit: sigma %.3e px over %d sources, lever arm %.1f px: matrix allowance %.3e'
                  % (sigma, n, lever, out['allowance']))
        print('%s: offset error %.3e px, matrix error %.3e, %d sources' % ((what,) + out[what]))
    _RUNS['r'] = out
    return out


def test_skysub_keeps_the_rejection_working_under_pedestals():
    r = three_runs()
    share = sum(r['skysub flagged'][:3]) / 3.0
    print('drawn hit pixels %.4f %% of frames 0..2, flagged with skysub %.4f %%' % (100 * r['drawn'], 100 * share))
    assert 0.0 < share < r['drawn'] + 0.005
    assert r['skysub'][0] <= r['yardstick'][0] + 2e-4
    assert r['skysub'][1] <= r['yardstick'][1] + r['allowance']


def test_without_skysub_the_pedestals_flag_most_of_the_last_frame():
    r = three_runs()
    print('frame 3 without skysub: %.2f %% flagged' % (100 * r['no skysub flagged'][3]))
    assert r['no skysub flagged'][3] > 0.5
