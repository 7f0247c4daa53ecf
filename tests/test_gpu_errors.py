"""The error measurements on the GPU (`subpixal_amd.detect.measure_errors`, spx_measure_errors_*) against the numpy
statement of tests/errors_statement.py: nhalf, fwhm (to the bit), flags and NaN pattern exactly, the four sums
within the derived float64 bounds; then the whole chain pixels -> DeviceImageCatalog -> weighted fit."""
import ctypes
import os
import sys

import numpy as np
import pytest

import errors_cases as ec
import errors_statement as es

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FIELD = {}


def field(dtype):
    """the 256 x 256 random field in `dtype`, its measure table from the device (what both sides read) and the
    statement, computed once and shared"""
    key = np.dtype(dtype).name
    if key not in _FIELD:
        from subpixal_amd import detect
        s = ec.field()
        a = dict(frame=np.ascontiguousarray(s['frame'], dtype), labels=s['labels'], n=s['n'], mask=s['mask'],
                 bkg=np.ascontiguousarray(s['bkg'], dtype), rms=np.ascontiguousarray(s['rms'], dtype), gain=s['gain'])
        table, flags, bbox = detect.measure(a['frame'], a['labels'], a['n'], background=a['bkg'], mask=a['mask'])
        a['table_device'] = table
        a['table'] = table.cpu().numpy()
        a['st'] = es.statement(a['frame'], a['labels'], a['n'], a['table'], a['rms'], bkg=a['bkg'], gain=a['gain'],
                               mask=a['mask'])
        for v in [a['table']] + list(a['st']['table'].values()) + list(a['st']['bound'].values()):
            v.setflags(write=False)                          # shared among the tests: nobody changes it
        _FIELD[key] = a
    return _FIELD[key]


def _measure(a, **over):
    from subpixal_amd import detect
    kw = dict(background=a['bkg'], gain=a['gain'], mask=a['mask'])
    kw.update(over)
    errors, eflags = detect.measure_errors(a['frame'], a['labels'], a['n'], a['table_device'], a['rms'], **kw)
    return errors.cpu().numpy(), eflags.cpu().numpy()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_random_field_against_the_statement(dtype):
    a = field(dtype)
    st = a['st']
    assert a['n'] > 150 and (st['flags'] & es.FLAG_NOISE).any() and (st['flags'] & es.FLAG_HALFMAX).any()
    assert (~st['flags'].astype(bool)).sum() > 50
    out, eflags = _measure(a)
    es.check(out, eflags, st, what='field 256x256 %s' % np.dtype(dtype).name)
    # without gain and with a scalar rms: other code paths of the same kernel
    st2 = es.statement(a['frame'], a['labels'], a['n'], a['table'], 0.0625, bkg=a['bkg'], gain=None, mask=a['mask'])
    from subpixal_amd import detect
    e2, f2 = detect.measure_errors(a['frame'], a['labels'], a['n'], a['table_device'], 0.0625, background=a['bkg'],
                                   mask=a['mask'])
    es.check(e2.cpu().numpy(), f2.cpu().numpy(), st2, what='field, scalar rms, no gain')


def test_small_scenes_against_the_statement():
    """the hand-placed scenes of the CPU tests, on the device"""
    from subpixal_amd import detect
    for name in sorted(ec.ALL):
        s = ec.ALL[name]()
        for dtype in (np.float32, np.float64):
            frame = np.ascontiguousarray(s['frame'], dtype)
            bkg = np.ascontiguousarray(s['bkg'], dtype) if np.ndim(s['bkg']) else s['bkg']
            rms = np.ascontiguousarray(s['rms'], dtype) if np.ndim(s['rms']) else s['rms']
            table, _, _ = detect.measure(frame, s['labels'], s['n'], background=bkg, mask=s['mask'])
            e, f = detect.measure_errors(frame, s['labels'], s['n'], table, rms, background=bkg, gain=s['gain'],
                                         mask=s['mask'])
            st = es.statement(frame, s['labels'], s['n'], table.cpu().numpy(), rms, bkg=bkg, gain=s['gain'],
                              mask=s['mask'])
            es.check(e.cpu().numpy(), f.cpu().numpy(), st, what='%s %s' % (name, np.dtype(dtype).name), verbose=False)


def test_determinism_bit_identical():
    import torch
    a = field(np.float32)
    runs = [_measure(a) for _ in range(4)]
    moved = dict(a, frame=torch.from_numpy(np.array(a['frame'])).cuda().clone(),
                 rms=torch.from_numpy(np.array(a['rms'])).cuda().clone())          # the same input at other addresses
    runs.append(_measure(moved))
    for e, f in runs[1:]:
        assert e.tobytes() == runs[0][0].tobytes() and f.tobytes() == runs[0][1].tobytes()


def test_c_abi_raw_pointers():
    import torch
    from subpixal_amd import _ffi, device
    device.init()
    lib = _ffi.load()
    a = field(np.float64)
    n = a['n']
    ny, nx = a['frame'].shape
    vp = ctypes.c_void_p
    dev = {k: torch.from_numpy(np.array(a[k])).cuda() for k in ('frame', 'labels', 'bkg', 'rms')}
    mask = torch.from_numpy(a['mask'].astype(np.uint8)).cuda()
    boxes = torch.empty((n + 1, 4), dtype=torch.int32, device='cuda')
    counts = torch.empty((n + 1,), dtype=torch.int32, device='cuda')
    assert lib.spx_label_bboxes_i32(vp(dev['labels'].data_ptr()), ny, nx, n, vp(boxes.data_ptr()),
                                    vp(counts.data_ptr()), None) == 0
    table = torch.empty((n, 13), dtype=torch.float64, device='cuda')
    flags = torch.empty((n,), dtype=torch.int32, device='cuda')
    assert lib.spx_measure_labels_f64(vp(dev['frame'].data_ptr()), vp(mask.data_ptr()), 0.0, vp(dev['bkg'].data_ptr()),
                                      vp(dev['labels'].data_ptr()), ny, nx, n, vp(boxes.data_ptr()),
                                      vp(table.data_ptr()), vp(flags.data_ptr()), None) == 0
    errors = torch.full((n + 1, 6), -7.0, dtype=torch.float64, device='cuda')
    eflags = torch.full((n + 1,), -7, dtype=torch.int32, device='cuda')

    def call(nlabels):
        return lib.spx_measure_errors_f64(vp(dev['frame'].data_ptr()), vp(mask.data_ptr()), 0.0,
                                          vp(dev['bkg'].data_ptr()), 0.0, vp(dev['rms'].data_ptr()), a['gain'],
                                          vp(dev['labels'].data_ptr()), ny, nx, nlabels, vp(boxes.data_ptr()),
                                          vp(table.data_ptr()), vp(errors.data_ptr()), vp(eflags.data_ptr()), None)
    assert call(0) == 0
    torch.cuda.synchronize()
    assert int((errors != -7.0).sum()) == 0 and int((eflags != -7).sum()) == 0       # no labels: nothing written
    assert call(n) == 0
    torch.cuda.synchronize()
    assert table.cpu().numpy().tobytes() == a['table'].tobytes()
    es.check(errors[:n].cpu().numpy(), eflags[:n].cpu().numpy(), a['st'], what='C ABI')
    assert float(errors[n, 0]) == -7.0 and int(eflags[n]) == -7                       # ... and no row beyond the last


def test_detect_sources_with_errors_equals_find_sources_with_its_rms():
    import torch
    from subpixal_amd import detect
    rng = np.random.default_rng(31)
    shape = (300, 340)
    f = 10.0 + rng.normal(0.0, 0.5, shape)
    for _ in range(25):
        f += ec.gauss(shape, rng.uniform(10, 290), rng.uniform(10, 330), rng.uniform(20, 200), rng.uniform(1.5, 3.0))
    f = f.astype(np.float32)
    kw = dict(min_area=5, deblend=True)
    plain = detect.detect_sources(f, nsigma=3.0, box=(32, 32), **kw)
    full = detect.detect_sources(f, nsigma=3.0, box=(32, 32), errors=True, gain=4.0, **kw)
    bg = full.background_model
    direct = detect.find_sources(f, bg.threshold(3.0), background=bg.background, rms=bg.rms, gain=4.0, **kw)
    assert len(full) == len(direct) == len(plain) >= 20
    assert torch.equal(full.segmentation, direct.segmentation) and torch.equal(full.segmentation, plain.segmentation)
    assert full.table_device.cpu().numpy().tobytes() == direct.table_device.cpu().numpy().tobytes()
    assert full.errors_device.cpu().numpy().tobytes() == direct.errors_device.cpu().numpy().tobytes()
    assert np.array_equal(full.flags, direct.flags)
    for c in ('fluxerr', 'fwhm', 'snr', 'pos_std', 'weight'):
        assert getattr(full, c).tobytes() == getattr(direct, c).tobytes(), c
    # errors=False: the same sources as before, and none of the new attributes or flag bits
    assert not plain.has_errors and not hasattr(plain, 'fluxerr') and 'fwhm' not in plain.table()
    assert plain.table_device.cpu().numpy().tobytes() == full.table_device.cpu().numpy().tobytes()
    mine = detect.FLAG_HALFMAX | detect.FLAG_NOISE
    assert np.array_equal(plain.flags, full.flags & ~mine) and not (plain.flags & mine).any()
    ok = np.isfinite(full.weight)
    assert ok.sum() >= 20 and np.all(full.snr[ok] > 3) and np.all((full.fwhm[ok] > 1) & (full.fwhm[ok] < 15))


# the margins of tests/test_gpu_detect.py::test_end_to_end_config5_with_noise, unchanged
FIT_MARGIN_OFFSET, FIT_MARGIN_MATRIX = 2.0e-4, 1.0e-7


def test_end_to_end_weighted_fit_from_pixels():
    """tools/align_catalog.py's scene at 1024^2 with 300 sources and noise of sigma 0.002 on both frames: the
    drizzled frame -> DeviceImageCatalog (background and noise maps, 5 sigma detection, errors, default filters) ->
    cutout_catalog(weight='pos_std') -> find_linear_fit(use_weights=True), beside the SAME catalogue with
    use_weights=False (the yardstick).  The weighted fit's offset and matrix errors may exceed the unweighted
    fit's own by at most FIT_MARGIN_OFFSET / FIT_MARGIN_MATRIX, the margins of test_end_to_end_config5_with_noise:
    its standard-error argument gives larger standard errors for the ~290 sources kept here than for the ~4900
    there, so these margins are the stricter choice on this scene; they are NOT rescaled by sqrt(4900 / kept).

    MEASURED on an MI355X by this test (float32, NCC; 295 sources detected, all 295 selected and cut out):
      unweighted: kept 293, offset error 5.80e-4 px, matrix error 8.40e-7
      weighted  : kept 284, offset error 2.23e-4 px, matrix error 5.18e-7
    The weighted fit is the closer one on this scene, so no rescaling of the margins is called for."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import align_catalog
    from subpixal_amd import blot, catalogs, cutout
    from subpixal_amd.align import find_linear_fit, iter_linear_fit
    noise, pad, margin = align_catalog.DETECT_NOISE, 3, 6
    s = align_catalog.build(size=1024, nsrc=300, noise=noise, detect=True)
    drz = torch.from_numpy(s['drz_frame']).cuda()
    cat = catalogs.DeviceImageCatalog(drz, nsigma=5.0, min_area=5)
    cat.execute()
    drz_cat = cat.cutout_catalog(drz, pad=pad + margin, weight='pos_std')
    n = len(drz_cat)
    assert 200 <= n <= len(cat.catalog['id']) <= len(cat.sources)
    sel = {int(i): k for k, i in enumerate(cat.catalog['id'])}
    rows = [sel[int(i)] for i in drz_cat.src_id]
    assert np.array_equal(drz_cat.src_weight, cat.catalog['weight'][rows])
    assert np.array_equal(drz_cat.src_pos, np.stack([cat.catalog['x'][rows], cat.catalog['y'][rows]], axis=1))
    assert np.all(np.isfinite(drz_cat.src_weight)) and np.all(drz_cat.src_weight > 0)
    assert drz_cat.src_weight.max() > 4 * drz_cat.src_weight.min()       # the weights do differ from source to source
    # the image-frame cutouts of the same sources, as align_catalog.build derives them from the drizzled boxes
    pos = drz_cat.src_pos
    pos2 = align_catalog.transform(s, pos)
    shift = np.round(pos2 - pos).astype(np.int32)
    iboxes = drz_cat.boxes - np.array([-margin, -margin, 2 * margin, 2 * margin], np.int32)
    iboxes[:, :2] += shift
    img_cat = cutout.CutoutCatalog(torch.from_numpy(s['img_cat']._frame_host).cuda(), iboxes, src_pos=pos2,
                                   src_id=drz_cat.src_id)
    affine = blot.shift_affine(n, x0=(shift[:, 0] + margin).astype(np.float64),
                               y0=(shift[:, 1] + margin).astype(np.float64))
    exact = iter_linear_fit(pos2 + 1.0, pos + 1.0, fitgeom='general', nclip=0)
    out = {}
    for name, use in (('unweighted', False), ('weighted', True)):
        fit, _, _ = find_linear_fit(img_cat, drz_cat, affine=affine, fitgeom='general', nclip=12, sigma=3.0,
                                    cc_type='NCC', use_weights=use)
        out[name] = (float(np.abs(fit['offset'] - exact['offset']).max()),
                     float(np.abs(fit['fit_matrix'] - exact['fit_matrix']).max()))
        print('%-10s: %d sources of %d detected, kept %d; offset err %.3e px, matrix err %.3e'
              % (name, n, len(cat.sources), fit['fitmask'].sum(), *out[name]))
    assert out['weighted'][0] <= out['unweighted'][0] + FIT_MARGIN_OFFSET
    assert out['weighted'][1] <= out['unweighted'][1] + FIT_MARGIN_MATRIX
