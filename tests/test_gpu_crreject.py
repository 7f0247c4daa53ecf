"""Cosmic-ray rejection on the device.

(a) Every case of tests/crreject_cases.py through the C entries (spx_drizzle_median_*, spx_drizzle_cr_*): `med`,
    `nmed` and `crmask` bit-identical to the kernel source run on CPU threads and `clean` identical off the mask, the
    single-frame values too; in any event against the numpy statement of tests/crreject_statement.py, as
    tests/test_crreject_cpu.py does, with the single-frame values taken from the device's own single-frame drizzles.
(b) `DeviceDrizzle(cr_reject=True)` on a 96 x 96, K = 3 scene with drawn hits.
(c) End to end on the scene of tests/test_gpu_drizzle_align.py (384 x 384, 81 sources, K = 4, frame 3 off by 0.3 px)
    with cosmic rays added to every frame: HITS hits of 1 .. 3 pixels per frame, amplitudes 0.3 .. 3 (a source peaks at
    0.5 .. 2), seed 41.  Three runs of the one-step fit of frame 3 against the drizzle of the other three: no hits;
    hits with cr_reject=False; hits with cr_reject=True.  The yardstick is the hit-free run: today's code path on the
    same noise.  The rejecting run must beat the non-rejecting one in offset and matrix error and stay within an
    allowance of the hit-free run.  On frames 0 .. 2, whose maps are exact, the share of flagged pixels must stay
    below the share of drawn hit pixels plus 0.5 % (a rejection that eats star cores would break it).

    The allowance.  The project's standing one is 2e-4 px / 1e-7 (test_gpu_detect.py, test_gpu_drizzle_align.py).
    The offset keeps it: the rejecting run is 1.4e-4 px off the hit-free one.  The matrix does not fit it: measured
    3.967e-6 against 1.543e-6, a difference of 2.4e-6.  That 1e-7 was derived for fits over ~4900 sources and a
    ~1200 px lever arm (test_gpu_detect.py: 3e-3 px / sqrt(4900) / 1200 px = 4e-8 per fit); this scene has 81
    sources on a ~92 px lever arm, where two fits over pixels that differ at all (here: ~300 replaced pixels per
    frame and the masked drops of the drizzle) differ by far more than 1e-7 whatever the code -- the same scene's
    two noise draws differ by 9e-7 (test_gpu_drizzle_align.py).  So, as test_gpu_detect.py derives its 4e-5 px, the
    matrix allowance is three standard errors of the difference of two fits, computed in the test from the
    HIT-FREE run's own per-source shift scatter and nothing of the rejecting run:
        sigma = the larger per-axis rms of the hit-free fit's residuals over its N kept sources
        L     = the rms distance per axis of those sources from their centre
        SE(matrix element of one fit) = sigma / (sqrt(N) L);   of the difference of two fits: sqrt(2) SE
        allowance = 3 sqrt(2) sigma / (sqrt(N) L)
    (printed by the test; measured sigma = 1.370e-3 px, N = 79, L = 91.6 px: 7.137e-6).

    Measured on an MI355X (offset error px / matrix error; DESIGN.md section 7 has the same):
        no hits                  9.257e-4 / 1.543e-6   (81 sources)
        hits, cr_reject=False    5.970e-2 / 9.247e-4   (200 "sources": the hits are detected too)
        hits, cr_reject=True     1.066e-3 / 3.967e-6   (81 sources)
        drawn hit pixels 0.2082 % of frames 0 .. 2, flagged 0.2118 %
    The statement alone, on the CPU (single-frame values from the drizzle on CPU threads), gives the same for this
    scene: 921 drawn hit pixels on frames 0 .. 2 (0.2082 %), 937 flagged (0.2118 %), no pixel under the margin.
"""
import os
import sys

import numpy as np
import pytest

import crreject_cases as cc
import crreject_emu as ce
import crreject_statement as cs
import drizzle_emu as de
import drizzle_statement as ds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

pytestmark = pytest.mark.gpu
DTYPES = (np.float32, np.float64)


def make(c, dtype, **over):
    from subpixal_amd import resample
    frames, weights, masks, shapes, maps, active, K = de.arrays(c, dtype)
    a = dict(frames=frames, maps=maps, out_shape=c['out_shape'], weights=weights, masks=masks, pixfrac=c['pixfrac'],
             kernel=c['kernel'], fill=c['fill'])
    a.update(over)
    return resample.DeviceDrizzle(**a)


def device_singles(d, c):
    """item 1 on the device: the existing drizzle with one frame active at a time"""
    K = len(c['frames'])
    NY, NX = c['out_shape']
    vals, valid = np.zeros((K, NY, NX), np.float32), np.zeros((K, NY, NX), bool)
    for k, on in enumerate(ce.actives(c)):
        if on:
            d._active = {n: n == k for n in range(K)}
            d._stale = True
            d.execute()
            valid[k] = ds.ctx_bits(d.output_ctx.cpu().numpy(), K)[k]
            vals[k] = np.where(valid[k], d.output_sci.cpu().numpy(), 0).astype(np.float32)
    d._active = {n: bool(a) for n, a in enumerate(ce.actives(c))}
    d._stale = True
    return vals, valid


_DEVICE = {}


def case_on_device(name, dtype):
    """a case of crreject_cases.ALL and its device_run, made once and shared by the tests of (a), which only read it"""
    key = (name, np.dtype(dtype).name)
    if key not in _DEVICE:
        c = cc.ALL[name]()
        _DEVICE[key] = (c,) + device_run(c, dtype)
    return _DEVICE[key]


def device_run(c, dtype):
    """the C entries through raw pointers: (vals, valid), (med, nmed), {k: (crmask, clean)}"""
    import torch
    from subpixal_amd import _ffi, device
    lib = _ffi.load()
    d = make(c, dtype)
    device.init()
    singles = device_singles(d, c)
    K = len(c['frames'])
    NY, NX = c['out_shape']
    p = ce.params(c)
    f32 = np.dtype(dtype) == np.float32
    rows = torch.from_numpy(d._pack(d._order, original=True)).cuda()
    med = torch.full((NY, NX), -77.0, dtype=torch.float32, device='cuda')
    nmed = torch.full((NY, NX), 201, dtype=torch.uint8, device='cuda')
    fn = lib.spx_drizzle_median_f32 if f32 else lib.spx_drizzle_median_f64
    _ffi.check(fn(rows.data_ptr(), K, sum(ce.actives(c)), ds.KERNELS[c['kernel']], p['nlow'], p['nhigh'], NY, NX,
                  med.data_ptr(), nmed.data_ptr(), device.stream_ptr()))
    fn = lib.spx_drizzle_cr_f32 if f32 else lib.spx_drizzle_cr_f64
    out = {}
    for k, on in enumerate(ce.actives(c)):
        if not on:
            continue
        ny, nx = c['frames'][k].shape
        rs, rm = ce.rms_args(c, k, dtype)
        rm = None if rm is None else torch.from_numpy(rm).cuda()
        crmask = torch.full((ny, nx), 201, dtype=torch.uint8, device='cuda')
        clean = torch.full((ny, nx), -77.0, dtype=torch.float32 if f32 else torch.float64, device='cuda')
        _ffi.check(fn(rows.data_ptr(), K, k, ny, nx, med.data_ptr(), nmed.data_ptr(), NY, NX, rs,
                      None if rm is None else rm.data_ptr(), float(p['sky']),
                      float('nan') if p['gain'] is None else float(p['gain']), p['snr'][0], p['snr'][1], p['scale'][0],
                      p['scale'][1], crmask.data_ptr(), clean.data_ptr(), device.stream_ptr()))
        out[k] = (crmask.cpu().numpy(), clean.cpu().numpy())
    return singles, (med.cpu().numpy(), nmed.cpu().numpy()), out


# ---------------------------------------------------------------------------------------------------------------
# (a)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', sorted(cc.ALL))
def test_case_against_the_statement(name, dtype):
    c, (vals, valid), (med, nmed), out = case_on_device(name, dtype)
    st = ce.statement(name, c, vals, valid, dtype)
    assert np.array_equal(nmed, st['nmed']), name
    assert med.tobytes() == st['med'].tobytes(), '%s: med differs at %d pixels' % (name, int((med != st['med']).sum()))
    tested = unsafe = 0
    for k, fs in enumerate(st['frames']):
        assert (fs is None) == (k not in out)
        if fs is not None:
            unsafe += cs.check_frame(*out[k], c['frames'][k], fs, dtype, '%s frame %d' % (name, k))
            tested += int(fs['testable'].sum())
    assert unsafe <= 0.01 * tested, (name, unsafe, tested)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', sorted(cc.ALL))
def test_bit_identical_to_the_kernels_on_cpu_threads(tmp_path_factory, name, dtype):
    emuz = ce.load(tmp_path_factory)
    c, (vals, valid), (med, nmed), out = case_on_device(name, dtype)
    evals, evalid = ce.singles(emuz, c, dtype)
    assert vals.tobytes() == evals.tobytes() and np.array_equal(valid, evalid)
    emed, enmed = ce.run_median(emuz, c, dtype)
    assert med.tobytes() == emed.tobytes() and nmed.tobytes() == enmed.tobytes(), name
    for k, (crmask, clean) in out.items():
        ecr, eclean = ce.run_cr(emuz, c, dtype, k, emed, enmed)
        assert crmask.tobytes() == ecr.tobytes(), (name, k)
        off = crmask == 0
        assert clean[off].tobytes() == eclean[off].tobytes(), (name, k)


@pytest.mark.parametrize('K', [65, 128])
def test_median_above_64_kib_of_lds(tmp_path_factory, K):
    """K * 1 KiB of dynamic LDS per workgroup: above 64 KiB the entry raises the kernel's limit first"""
    c = cc.many(K)
    (vals, valid), (med, nmed), out = device_run(c, np.float32)
    exp_med, exp_nmed = cs.median(vals, valid)
    assert int(nmed.max()) == K and np.array_equal(nmed, exp_nmed) and med.tobytes() == exp_med.tobytes()
    emed, enmed = ce.run_median(ce.load(tmp_path_factory), c, np.float32)
    assert med.tobytes() == emed.tobytes() and nmed.tobytes() == enmed.tobytes()
    assert out[0][0][3, 3] == 1


# ---------------------------------------------------------------------------------------------------------------
# (b)
# ---------------------------------------------------------------------------------------------------------------
def add_hits(frames, rng, nhits, lo, hi):
    """`nhits` cosmic rays of 1 .. 3 pixels (a straight run in x, y or along a diagonal) per frame, amplitudes lo .. hi
    (the later pixels of a run fainter); returns the new frames and per frame the list of (j, i, amplitude)"""
    out, drawn = [], []
    for f in frames:
        f = f.copy()
        ny, nx = f.shape
        amps = {}
        for _ in range(nhits):
            j, i = int(rng.integers(2, ny - 2)), int(rng.integers(2, nx - 2))
            dj, di = [(0, 1), (1, 0), (1, 1), (1, -1)][int(rng.integers(4))]
            a = rng.uniform(lo, hi)
            for q in range(int(rng.integers(1, 4))):
                p = (min(max(j + q * dj, 0), ny - 1), min(max(i + q * di, 0), nx - 1))
                amps[p] = amps.get(p, 0.0) + a * (1.0 if q == 0 else rng.uniform(0.3, 0.9))
        for (j, i), a in amps.items():
            f[j, i] = f.dtype.type(f[j, i] + a)
        out.append(f)
        drawn.append([(j, i, float(out[-1][j, i]) - float(frames[len(out) - 1][j, i])) for (j, i) in amps])
    return out, drawn


def test_device_drizzle_with_cr_reject():
    import bench_drizzle as bd
    from subpixal_amd import resample
    N, K = 96, 3
    s = bd.dither_scene(N, 9, K, seed=3, sigma=2.5, border=20.0)
    frames, drawn = add_hits(s['frames'], np.random.default_rng(17), 12, 0.05, 1.0)
    maps = np.stack(s['truth'])
    mask0 = np.zeros((N, N), np.uint8)
    mask0[40:44, 10:30] = 1
    masks = [mask0, None, None]
    d = resample.DeviceDrizzle(frames, maps, (N, N), masks=masks, cr_reject=True, rms=s['noise']).execute()
    assert len(d.output_crclean) == K == len(d.output_crmask) and d.output_median.shape == (N, N)
    assert d.output_nmedian.dtype.is_floating_point is False and int(d.output_nmedian.max()) == K
    crm = [m.cpu().numpy() for m in d.output_crmask]
    assert all(d.crmask(k) is d.output_crmask[k] and d.crclean(k) is d.output_crclean[k] for k in range(K))
    # the statement, from the device's own single-frame drizzles
    c = dict(frames=[f.astype(np.float64) for f in frames], maps=list(maps), out_shape=(N, N), weights=None,
             masks=masks, active=None, pixfrac=1.0, kernel='square', fill=0.0, rms=K * [s['noise']], cr={})
    vals, valid = device_singles(resample.DeviceDrizzle(frames, maps, (N, N), masks=masks), c)
    st = cs.statement(c, vals, valid)
    assert d.output_median.cpu().numpy().tobytes() == st['med'].tobytes()
    strong = flagged = 0
    for k in range(K):
        fs = st['frames'][k]
        cs.check_frame(crm[k], d.output_crclean[k].cpu().numpy(), frames[k], fs, np.float32, 'frame %d' % k)
        for j, i, a in drawn[k]:
            if fs['testable'][j, i] and a > 2.0 * fs['thr'][0][j, i]:
                strong += 1
                flagged += int(crm[k][j, i])
    print('%d of %d drawn hit pixels exceed twice their test-1 threshold; %d flagged' % (
        strong, sum(len(h) for h in drawn), flagged))
    assert strong >= 20 and flagged == strong
    # the final drizzle is the plain drizzle over the merged masks
    merged = [crm[k] | (0 if masks[k] is None else masks[k]) for k in range(K)]
    plain = resample.DeviceDrizzle(frames, maps, (N, N), masks=merged).execute()
    for a, b in ((d.output_sci, plain.output_sci), (d.output_wht, plain.output_wht), (d.output_ctx, plain.output_ctx)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert plain.output_crclean is None
    # a fast replace keeps the masks; a second full execute() after the data changed makes new ones
    q = d.copy()
    q.fast_drop_image(2)
    assert q.crmask(0) is d.crmask(0) and q.output_sci is not None
    two = resample.DeviceDrizzle(frames[:2], maps[:2], (N, N), masks=merged[:2]).execute()
    assert q.output_sci.cpu().numpy().tobytes() == two.output_sci.cpu().numpy().tobytes()
    j, i, _ = drawn[1][0]
    d._pool[1].data[j, i] -= drawn[1][0][2]                        # the hit is gone from the resident frame
    before = d.crmask(1)
    d.execute()
    assert d.crmask(1) is not before and int(before[j, i]) == 1 and int(d.crmask(1)[j, i]) == 0
    # with the feature off nothing of it is there
    off = resample.DeviceDrizzle(frames, maps, (N, N), masks=masks).execute()
    assert off.output_crclean is None and off.output_median is None and off.crclean(0) is None


# ---------------------------------------------------------------------------------------------------------------
# (c)
# ---------------------------------------------------------------------------------------------------------------
HITS = 150
_RUNS = {}


def three_runs():
    """{'clean' | 'hits' | 'rejected': (offset error, matrix error, sources)}, the drawn and the flagged share, the
    matrix allowance"""
    import test_gpu_drizzle_align as ta
    from subpixal_amd import align, resample
    if 'r' in _RUNS:
        return _RUNS['r']
    s = ta.scene()
    SIZE = ta.SIZE
    maps = [m.copy() for m in s['truth']]
    maps[3] = ta.perturbed(s['truth'], 3)
    hit_frames, drawn = add_hits(s['frames'], np.random.default_rng(41), HITS, 0.3, 3.0)
    got, share, allowance = {}, None, None
    for what, frames, kw in (('clean', s['frames'], {}), ('hits', hit_frames, {}),
                             ('rejected', hit_frames, dict(cr_reject=True, rms=s['noise']))):
        drz = resample.DeviceDrizzle(frames, np.stack(maps), (SIZE, SIZE), **kw)
        if kw:
            drz.execute()                                     # the full execute(): masks and cleaned frames
            npix = sum(len(h) for h in drawn[:3])
            nflag = sum(int(drz.crmask(k).sum()) for k in range(3))
            share = (npix / (3.0 * SIZE * SIZE), nflag / (3.0 * SIZE * SIZE))
        q = drz.copy()
        q.fast_drop_image(3)
        cat = ta.catalog()
        cat.set_image(q.output_sci)
        cat.execute()
        prim = cat.cutout_catalog(q.output_sci, pad=1, weight='pos_std')
        img_cat, drz_cat, aff = align._frame_catalogs(q, 3, prim, 6, np.float32)
        fit, _, _ = align.find_linear_fit(img_cat, drz_cat, affine=aff, fitgeom='general', nclip=3, sigma=3.0)
        got[what] = ta.errors(align.compose_fit(maps[3], fit), s['truth'][3]) + (len(img_cat),)
        if what == 'clean':                                   # the yardstick's own scatter: the module docstring
            keep = np.asarray(fit['fitmask'], bool)
            pos = np.asarray(img_cat.src_pos, np.float64)[keep]
            sigma, n = float(np.max(fit['rms'])), int(keep.sum())
            lever = float(np.sqrt(np.mean(np.var(pos, axis=0))))
            allowance = 3.0 * np.sqrt(2.0) * sigma / (np.sqrt(n) * lever)
            print('hit-free fit: sigma %.3e px over %d sources, lever arm %.1f px: matrix allowance %.3e'
                  % (sigma, n, lever, allowance))
        print('%s: offset error %.3e px, matrix error %.3e, %d sources' % ((what,) + got[what]))
    print('drawn hit pixels %.4f %% of frames 0..2, flagged %.4f %%' % (100 * share[0], 100 * share[1]))
    _RUNS['r'] = got, share, allowance
    return _RUNS['r']


def test_rejecting_beats_not_rejecting():
    got, _, _ = three_runs()
    assert got['rejected'][0] < got['hits'][0] and got['rejected'][1] < got['hits'][1]


def test_rejecting_stays_within_the_allowance_of_the_hit_free_run():
    got, _, matrix_allowance = three_runs()
    assert got['rejected'][0] <= got['clean'][0] + 2e-4
    assert got['rejected'][1] <= got['clean'][1] + matrix_allowance


def test_the_rejection_does_not_eat_star_cores():
    _, (drawn, flagged), _ = three_runs()
    assert 0.0 < flagged < drawn + 0.005
