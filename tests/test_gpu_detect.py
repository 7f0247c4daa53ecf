"""Source finding on the GPU (`subpixal_amd.detect`, spx_detect_label_* / spx_measure_labels_*) against the
numpy/scipy statement of tests/detect_statement.py: label images integer for integer, measurements within the
derived float64 summation bounds.  These are the tests that prove the merge ACROSS workgroups on real hardware
(the CPU harness of tests/test_detect_cpu.py runs workgroups one after another)."""
import ctypes
import os
import sys

import numpy as np
import pytest
from scipy import ndimage

import detect_statement as ds

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_WORKSPACE = -4


def random_field(ny, nx, seed, dtype, smooth=2.5):
    """smoothed white noise with unit variance: thousands of blobby components above a threshold near 1"""
    rng = np.random.default_rng(seed)
    f = ndimage.gaussian_filter(rng.standard_normal((ny, nx)), smooth, mode='wrap')
    return (f / f.std()).astype(dtype)


def snake(ny, nx, dtype, seed=1):
    """one 1-pixel-wide rectangular spiral (arms 2 px apart) over the whole frame: a single component that passes
    through every tile, whose root is pixel 0"""
    rng = np.random.default_rng(seed)
    on = np.zeros((ny, nx), bool)
    y0, x0, y1, x1 = 0, 0, ny - 1, nx - 1
    while x1 - x0 >= 2 and y1 - y0 >= 2:
        on[y0, x0:x1 + 1] = True
        on[y0:y1 + 1, x1] = True
        on[y1, x0 + 2:x1 + 1] = True
        on[y0 + 2:y1 + 1, x0 + 2] = True
        y0, x0, y1, x1 = y0 + 2, x0 + 2, y1 - 2, x1 - 2
        on[y0, x0] = True
    return np.where(on, np.round(rng.uniform(2, 6, on.shape) * 1024) / 1024, 0.0).astype(dtype)


def _run(frame, thr, bkg=0.0, mask=None, filt=None, min_area=1, conn=8):
    from subpixal_amd import detect
    src = detect.find_sources(frame, thr, background=bkg, mask=mask, filter_kernel=filt, min_area=min_area,
                              connectivity=conn)
    return src, (src.segmentation.cpu().numpy(), src.table_device.cpu().numpy(), src.flags, src.bbox)


def untie(frame, thr, mask=None, filt=None, **_):
    """Scene construction: moves the few pixels whose (filtered) value lies within rounding of the threshold in
    the float64 statement away from it, so that no pixel's detection is left to float32 rounding."""
    for _ in range(20):
        tie = ds.detection(frame, thr, mask, filt)[1]
        if not tie.any():
            return frame
        frame[tie] += np.asarray(0.01, frame.dtype)
    raise AssertionError("could not clear the threshold ties")


def _check(what, frame, thr, **kw):
    frame = untie(frame, thr, **kw)
    st = ds.statement(frame, thr, **kw)
    src, got = _run(frame, thr, **kw)
    res = ds.check(*got, st, what=what)
    assert len(src) == st['n']
    return src, st


K3 = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]]) / 16.0
K75 = np.outer(np.exp(-0.5 * (np.arange(-3, 4) / 1.5) ** 2), np.exp(-0.5 * (np.arange(-2, 3) / 1.0) ** 2))
K75 = K75 / K75.sum()
K75[0, 0] = -K75[0, 0]                                      # not symmetric: a convolution would differ


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_random_fields_against_scipy(dtype):
    f = random_field(2048, 3000, 11, dtype)
    for conn in (8, 4):
        for min_area in (3, 12):
            src, st = _check('field 2048x3000 conn %d min_area %d %s' % (conn, min_area, np.dtype(dtype)), f, 1.1,
                             conn=conn, min_area=min_area, bkg=-4.0)
            assert st['n'] > 2000
    g = random_field(1531, 2047, 12, dtype)
    rng = np.random.default_rng(13)
    mask = ndimage.binary_dilation(rng.random(g.shape) < 2e-4, iterations=2)
    g[rng.random(g.shape) < 1e-4] = np.nan
    g[rng.random(g.shape) < 5e-5] = np.inf
    thr_map = (1.0 + 0.3 * np.sin(np.arange(g.shape[1]) / 200.0))[None, :] * np.ones(g.shape)
    bkg_map = np.full(g.shape, -5.0, dtype) + (np.arange(g.shape[0]) % 7)[:, None].astype(dtype) / 8
    _check('field masked, threshold map, background map', g, thr_map.astype(np.float32), mask=mask, min_area=4,
           bkg=bkg_map)
    _check('field masked, 3x3 filter', g, 0.9, mask=mask, filt=K3.astype(dtype), min_area=4, bkg=-5.0)
    _check('field 7x5 filter conn 4', g, 0.8, filt=K75.astype(dtype), min_area=6, conn=4, bkg=-5.0)
    # without min_area: every component stays, single pixels included (a single pixel has no direction, so the
    # smoothing is chosen such that they stay below the theta cap)
    _check('field min_area 1', random_field(1201, 1603, 14, dtype, smooth=4.0), 1.3, min_area=1, bkg=-5.0)


@pytest.mark.parametrize('conn', [8, 4])
def test_one_component_through_every_tile(conn):
    f = snake(1023, 1501, np.float32)
    src, st = _check('snake conn %d' % conn, f, 1.0, conn=conn)
    assert st['n'] == 1 and len(src) == 1 and src.npix[0] == int((f > 0).sum())
    # all of the frame detected: one component, every tile border merges
    full = random_field(515, 1030, 15, np.float64) + 10.0
    src, st = _check('full frame', full, 1.0, conn=conn)
    assert st['n'] == 1 and src.npix[0] == full.size
    src, st = _check('empty frame', full, 100.0, conn=conn)
    assert len(src) == 0 and int(src.segmentation.max()) == 0


def test_determinism_bit_identical():
    import torch
    from subpixal_amd import detect
    f = random_field(1777, 2311, 16, np.float32)
    mask = np.random.default_rng(17).random(f.shape) < 1e-3
    fd = torch.from_numpy(f).cuda()
    runs = []
    for i in range(6):
        if i == 5:                                          # the same input at another address
            keep = fd
            fd = torch.empty_like(keep)
            fd.copy_(keep)
            assert fd.data_ptr() != keep.data_ptr()
        src = detect.find_sources(fd, 1.05, background=-4.0, mask=mask, filter_kernel=K3, min_area=3)
        runs.append((src.segmentation.cpu().numpy().tobytes(), src.table_device.cpu().numpy().tobytes(),
                     src.flags.tobytes(), src.bbox.tobytes(), len(src)))
    assert runs[0][4] > 2000
    for r in runs[1:]:
        assert r == runs[0]


def test_c_abi_raw_pointers_and_short_workspace():
    import torch
    from subpixal_amd import _ffi, device
    device.init()
    lib = _ffi.load()
    f = untie(random_field(301, 517, 18, np.float32), 1.0)
    st = ds.statement(f, 1.0, min_area=2)
    ny, nx = f.shape
    fd = torch.from_numpy(f).cuda()
    need = lib.spx_detect_workspace_bytes(ny, nx)
    assert need >= 8 * ny * nx
    work = torch.full((need,), 0x5A, dtype=torch.uint8, device='cuda')
    labels = torch.full((ny, nx), -77, dtype=torch.int32, device='cuda')
    nlab = torch.full((1,), -77, dtype=torch.int32, device='cuda')
    vp = ctypes.c_void_p
    # one byte short: refused, nothing written
    rc = lib.spx_detect_label_f32(vp(fd.data_ptr()), None, 1.0, None, None, 1, 1, ny, nx, 8, 2, vp(work.data_ptr()),
                                  need - 1, vp(labels.data_ptr()), vp(nlab.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == E_WORKSPACE
    assert b'workspace' in lib.spx_last_error()
    assert int((labels != -77).sum()) == 0 and int(nlab[0]) == -77 and int((work != 0x5A).sum()) == 0
    rc = lib.spx_detect_label_f32(vp(fd.data_ptr()), None, 1.0, None, None, 1, 1, ny, nx, 8, 2, None, need,
                                  vp(labels.data_ptr()), vp(nlab.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == E_WORKSPACE and int((labels != -77).sum()) == 0 and int(nlab[0]) == -77
    # the full call on the default stream, then boxes and measurements, all through raw pointers
    rc = lib.spx_detect_label_f32(vp(fd.data_ptr()), None, 1.0, None, None, 1, 1, ny, nx, 8, 2, vp(work.data_ptr()),
                                  need, vp(labels.data_ptr()), vp(nlab.data_ptr()), None)
    assert rc == 0
    torch.cuda.synchronize()
    n = int(nlab[0])
    assert n == st['n']
    boxes = torch.empty((n + 1, 4), dtype=torch.int32, device='cuda')
    counts = torch.empty((n + 1,), dtype=torch.int32, device='cuda')
    assert lib.spx_label_bboxes_i32(vp(labels.data_ptr()), ny, nx, n, vp(boxes.data_ptr()), vp(counts.data_ptr()),
                                    None) == 0
    table = torch.empty((n, 13), dtype=torch.float64, device='cuda')
    flags = torch.empty((n,), dtype=torch.int32, device='cuda')
    assert lib.spx_measure_labels_f32(vp(fd.data_ptr()), None, -3.0, None, vp(labels.data_ptr()), ny, nx, n,
                                      vp(boxes.data_ptr()), vp(table.data_ptr()), vp(flags.data_ptr()), None) == 0
    torch.cuda.synchronize()
    ds.check(labels.cpu().numpy(), table.cpu().numpy(), flags.cpu().numpy(), boxes[1:].cpu().numpy(),
             ds.statement(f, 1.0, min_area=2, bkg=-3.0), what='C ABI')


# the margin of test_end_to_end_config5 (see its docstring)
FIT_MARGIN_OFFSET, FIT_MARGIN_MATRIX = 2.0e-4, 1.0e-7


def test_end_to_end_config5_with_noise():
    """BASELINE config 5 (4096^2, 5000 sources) with Gaussian noise of sigma 0.002 on both frames:
    find_sources(drizzled frame, 5 sigma, min_area 5) -> cutout_catalog -> find_linear_fit, beside the existing
    path on the drawn segmentation and the true positions (the yardstick), same scene, same process.

    MEASURED on an MI355X by this test before the margins were set (float32, NCC):
      drawn   : 5000 sources, 4923 kept, offset error 8.04e-4 px, matrix error 1.95e-7
      detected: 4921 sources, 4878 kept, offset error 8.63e-4 px, matrix error 2.04e-7
      (4027 isolated sources, each detected exactly once; |detected (x, y) - truth| median 0.0043 px, 99 % 0.017 px)
    The margins FIT_MARGIN_OFFSET = 2e-4 px and FIT_MARGIN_MATRIX = 1e-7 are what the detected path's fit error may
    exceed the drawn path's own by.  Reason: each fit averages ~4900 per-source shifts whose noise-driven scatter
    is ~3e-3 px rms (median 2.2e-3, 90 % 5e-3 in both paths), so its offset carries a standard error of
    3e-3 / sqrt(4900) = 4e-5 px and its matrix that over the ~1200 px rms lever arm, 4e-8.  The two paths see the same
    noise through different segment shapes and source subsets, so their errors differ by an amount of that size
    (measured: +5.9e-5 px, +0.9e-8); the margins allow about three standard errors of the difference and stay
    a factor 4 below the drawn path's own error.  The drawn path is the yardstick, the detected path is not."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import align_catalog
    from subpixal_amd.align import find_linear_fit, iter_linear_fit
    noise, pad, margin = align_catalog.DETECT_NOISE, 3, 6
    drawn = align_catalog.build(noise=noise)
    det = align_catalog.build(noise=noise, detect=True)
    assert np.array_equal(drawn['drz_frame'], det['drz_frame'])
    src = det['src']
    xy, big = det['xy_all'], det['big_all']
    # isolated: compact, no other source within 40 px (compact segments reach 17 px, the detection isophote of the
    # brightest compact source 2.0 exp(-r^2/32) = 0.01 lies at r = 13 px), and clear of the extended ones' reach
    from scipy.spatial import cKDTree
    tree = cKDTree(xy)
    d2 = tree.query(xy, k=2)[0][:, 1]
    near_big = np.zeros(len(xy), bool)
    if big.any():
        near_big = cKDTree(xy[big]).query(xy, k=1)[0] < 80.0
    iso = (~big) & (d2 > 40.0) & ~near_big
    assert iso.sum() > 1000
    det_tree = cKDTree(np.stack([src.x, src.y], axis=1)[np.isfinite(src.x)])
    counts = np.array([len(c) for c in det_tree.query_ball_point(xy[iso], 3.0)])
    print('isolated sources %d of %d; detected exactly once %d, never %d, more than once %d; %d detections in all'
          % (iso.sum(), len(xy), (counts == 1).sum(), (counts == 0).sum(), (counts > 1).sum(), len(src)))
    assert np.all(counts == 1)
    dist, _ = det_tree.query(xy[iso], k=1)
    print('isolated sources: |detected (x, y) - truth| median %.4f px, 99%% %.4f px' % (
        np.median(dist), np.percentile(dist, 99)))
    # the catalog find_linear_fit gets is the one Sources.cutout_catalog builds
    drz_cat = src.cutout_catalog(torch.from_numpy(det['drz_frame']).cuda(), pad=pad + margin)
    assert np.array_equal(np.asarray(drz_cat.boxes), np.asarray(det['drz_cat'].boxes))
    assert np.array_equal(np.asarray(drz_cat.src_pos), det['xy'])
    out = {}
    for name, s, cat in (('drawn', drawn, drawn['drz_cat']), ('detected', det, drz_cat)):
        fit, _, _ = find_linear_fit(s['img_cat'], cat, affine=s['affine'], fitgeom='general', nclip=12, sigma=3.0,
                                    cc_type='NCC')
        exact = iter_linear_fit(s['xy2'] + 1.0, s['xy'] + 1.0, fitgeom='general', nclip=0)
        err = np.abs(fit['subpixal_img_dxy'] - (s['xy'] - s['xy2'])).max(axis=1)
        out[name] = (float(np.abs(fit['offset'] - exact['offset']).max()),
                     float(np.abs(fit['fit_matrix'] - exact['fit_matrix']).max()))
        print('%-8s: %d sources, kept %d; |shift - truth| median %.2e 90%% %.2e px; offset err %.3e px, matrix err '
              '%.3e' % (name, len(err), fit['fitmask'].sum(), np.median(err), np.percentile(err, 90), *out[name]))
    assert out['detected'][0] <= out['drawn'][0] + FIT_MARGIN_OFFSET
    assert out['detected'][1] <= out['drawn'][1] + FIT_MARGIN_MATRIX
