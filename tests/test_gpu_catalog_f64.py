"""The catalog path (CutoutCatalog + find_linear_fit) on float64 frames: the reference computes in the cutouts'
dtype (cutout.py:698-701, blot.py:155, cc.py:121-156), so a float64 catalog gathers, blots and normalises in
float64 and each source equals cc.find_displacement on its own float64 Cutout objects, bit for bit."""
import os
import sys

import numpy as np
import pytest

from oracle import subpixal_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

TOL64 = 3e-5          # float64 cutouts against the float64 oracle (the repo's float64-golden tolerance)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _blots64(dzct, aff, shape):
    """the four blots of a drizzled Cutout the way the list path makes them: masked pixels zeroed in the
    cutout's dtype (align.py:661), resampled in float32 (blot.py:134), stored in the image cutout's float64
    (blot.py:155)"""
    from subpixal_amd import blot
    d = np.where(dzct.mask, 0.0, dzct.data)
    return blot.blot_affine4_batch(d[None].astype(np.float32), aff, shape)[0].astype(np.float64)


def test_f64_catalog_gather_equals_its_cutouts():
    from subpixal_amd.cutout import CutoutCatalog
    rng = np.random.default_rng(21)
    frame = 1.0 + rng.integers(1, 2 ** 20, (120, 150)) * 2.0 ** -40          # float32 cannot hold these
    frame[::4] = rng.standard_normal((30, 150)) * 1e4
    frame[40, 60], frame[41, 61] = np.nan, -np.inf
    seg = np.zeros((120, 150), np.int32)
    seg[30:70, 40:90] = 1
    seg[50:60, 70:80] = 2
    mask = np.zeros((120, 150), bool)
    mask[35, 45] = True
    boxes = np.array([[38, 28, 55, 45], [-5, 100, 30, 25], [140, -4, 14, 12]], np.int32)
    cat = CutoutCatalog(frame, boxes, mask=mask, segmentation_image=seg, src_id=[1, 7, 2], dtype=np.float64)
    assert cat.dtype == np.float64 and cat.frame.dtype.is_floating_point and cat.frame.element_size() == 8
    for zero_masked in (True, False):
        packed, offs, _ = cat.packed(zero_masked=zero_masked)
        assert packed.dtype.itemsize == 8
        packed, offs = packed.cpu().numpy(), offs.cpu().numpy()
        for k in range(len(boxes)):
            ct = cat[k]
            assert ct.data.dtype == np.float64
            want = np.where(ct.mask, 0.0, ct.data) if zero_masked else ct.data
            got = packed[offs[k]:offs[k] + want.size].reshape(want.shape)
            if zero_masked:
                assert _same_bits(got, want), k
            else:        # raw: the cutouts' data (non-finite frame pixels become the fill, as in float32)
                fin = np.isfinite(ct.data)
                assert np.array_equal(np.isnan(got), ~fin) and _same_bits(got[fin], ct.data[fin]), k
    v = packed[np.isfinite(packed)]
    assert np.count_nonzero(v != v.astype(np.float32)) > 0.3 * v.size
    # float32 is the default: a float64 frame still gives float32 buffers and items
    c32 = CutoutCatalog(frame, boxes)
    p32, _, _ = c32.packed()
    assert p32.dtype.itemsize == 4 and c32[0].data.dtype == np.float32 and c32.dtype == np.float32
    # a float32 frame is widened for float64
    c = CutoutCatalog(frame.astype(np.float32), boxes, dtype=np.float64)
    assert c.packed()[0].dtype.itemsize == 8 and c[0].data.dtype == np.float64
    with pytest.raises(ValueError, match="float32 or float64"):
        CutoutCatalog(frame, boxes, dtype=np.float16)


def _branch_scene(dt):
    """the scene of test_gpu_align.py's every-family test: a source of every kernel family, one above 128 px
    (general path), a NaN pixel and a 2-pixel-wide cutout -- rendered in float64"""
    rng = np.random.default_rng(6)
    size = 700
    xy = np.array([[80, 90], [200, 120], [350, 140], [520, 160], [200, 450], [480, 480], [620, 60]],
                  np.float64) + rng.uniform(-0.4, 0.4, (7, 2))
    wh = np.array([[30, 20], [44, 40], [66, 70], [90, 100], [150, 140], [40, 40], [2, 30]])
    t = np.array([0.6, -0.9])
    drz = np.zeros((size, size))
    img = np.full((size, size), 0.0)
    yy, xx = np.mgrid[:size, :size].astype(np.float64)
    for k, (x, y) in enumerate(xy):
        s = 2.5 + 0.8 * k
        drz += np.exp(-((xx - x) ** 2 + (yy - y) ** 2) / (2 * s * s))
        img += np.exp(-((xx - x - t[0]) ** 2 + (yy - y - t[1]) ** 2) / (2 * s * s))
    img[int(xy[5, 1]), int(xy[5, 0])] = np.nan
    boxes = np.stack([np.round(xy[:, 0]).astype(int) - wh[:, 0] // 2, np.round(xy[:, 1]).astype(int) - wh[:, 1] // 2,
                      wh[:, 0], wh[:, 1]], axis=1).astype(np.int32)
    return img.astype(dt), drz.astype(dt), boxes, xy, wh, t


@pytest.mark.parametrize('cc_type', ['NCC', 'ZNCC'])
def test_f64_catalog_every_branch_bit_identical_to_cutouts(cc_type):
    from subpixal_amd import blot
    from subpixal_amd.align import find_linear_fit, ST_SKIPPED
    from subpixal_amd.cutout import CutoutCatalog
    img, drz, boxes, xy, wh, t = _branch_scene(np.float64)
    m = 8
    dboxes = boxes + np.array([-m, -m, 2 * m, 2 * m], np.int32)
    img_cat = CutoutCatalog(img, boxes, src_pos=xy + t, dtype=np.float64)
    drz_cat = CutoutCatalog(drz, dboxes, src_pos=xy, src_weight=np.ones(7), dtype=np.float64)
    aff = blot.shift_affine(7, x0=float(m), y0=float(m))
    fit, iccs, blts = find_linear_fit(img_cat, drz_cat, affine=aff, fitgeom='shift', cc_type=cc_type)
    d, st = fit['subpixal_img_dxy'], fit['subpixal_status']
    assert list(st) == [0, 0, 0, 0, 0, 6, ST_SKIPPED]
    assert not fit['fitmask'][5] and not fit['fitmask'][6] and fit['fitmask'][:5].all()
    from subpixal_amd import cc
    for k in range(6):
        imct, dzct = img_cat[k], drz_cat[k]
        assert imct.data.dtype == np.float64 and dzct.data.dtype == np.float64
        b = _blots64(dzct, aff[k:k + 1], imct.data.shape)
        dx, dy, icc, _ = cc.find_displacement(imct.data, b[0], b[1], b[2], b[3], cc_type=cc_type, full_output=True)
        if k == 5:
            assert not (np.isfinite(dx) and np.isfinite(dy)) or (dx, dy) == (d[k, 0], d[k, 1])
            continue
        assert dx == d[k, 0] and dy == d[k, 1], (k, dx - d[k, 0], dy - d[k, 1])
        assert icc.dtype == np.float64 and iccs[k].dtype == np.float64 and blts[k].dtype == np.float64
        assert _same_bits(icc, iccs[k]) and _same_bits(b[0], blts[k]), k
    if cc_type == 'NCC':
        np.testing.assert_allclose(d[:5], np.tile(-t, (5, 1)), atol=5e-3)
    # the same maps as degree-2 polynomials (the poly branch of the blot kernel)
    coef = np.zeros((7, 2, 21))
    for k in range(7):
        coef[k, 0, 0] = (wh[k, 0] - 1) / 2.0 + m
        coef[k, 1, 0] = (wh[k, 1] - 1) / 2.0 + m
        coef[k, 0, 1] = 1.0
        coef[k, 1, 2] = 1.0
    fit2, i2, b2 = find_linear_fit(img_cat, drz_cat, poly=(coef, 2), fitgeom='shift', cc_type=cc_type)
    np.testing.assert_allclose(fit2['subpixal_img_dxy'][:5], d[:5], atol=2e-5)
    assert list(fit2['subpixal_status']) == list(st) and i2[0].dtype == np.float64 and b2[0].dtype == np.float64


PEDESTAL = 1.0e4      # image sky level; the sources on it are 0.1..0.3 high


def _pedestal_scene(n=12, size=400, seed=41):
    """ZNCC's case for float64: faint sources on a large image sky level (float32 keeps ~1e-3 of 1e4, a few
    per cent of a source) against a sky-subtracted drizzled frame"""
    rng = np.random.default_rng(seed)
    g = int(np.ceil(np.sqrt(n)))
    cell = (size - 80) / g
    xy = np.array([[40 + (k % g + 0.5) * cell, 40 + (k // g + 0.5) * cell] for k in range(n)]) + \
        rng.uniform(-3, 3, (n, 2))
    t = np.array([0.37, -0.61])
    a = rng.uniform(0.1, 0.3, n)
    s = rng.uniform(2.5, 4.0, n)
    yy, xx = np.mgrid[:size, :size].astype(np.float64)
    drz = np.zeros((size, size))
    img = np.full((size, size), PEDESTAL)
    for k in range(n):
        drz += a[k] * np.exp(-((xx - xy[k, 0]) ** 2 + (yy - xy[k, 1]) ** 2) / (2 * s[k] ** 2))
        img += a[k] * np.exp(-((xx - xy[k, 0] - t[0]) ** 2 + (yy - xy[k, 1] - t[1]) ** 2) / (2 * s[k] ** 2))
    w = 2 * np.round(3 * s).astype(int) + 1 + rng.integers(0, 8, n)
    boxes = np.stack([np.round(xy[:, 0]).astype(int) - w // 2, np.round(xy[:, 1]).astype(int) - w // 2, w, w],
                     axis=1).astype(np.int32)
    return img, drz, boxes, xy, t


def test_f64_catalog_matches_the_float64_oracle_where_float32_does_not():
    from subpixal_amd import blot
    from subpixal_amd.align import find_linear_fit
    from subpixal_amd.cutout import CutoutCatalog
    img, drz, boxes, xy, t = _pedestal_scene()
    m = 8
    n = len(boxes)
    dboxes = boxes + np.array([-m, -m, 2 * m, 2 * m], np.int32)
    img_cat = CutoutCatalog(img, boxes, src_pos=xy + t, dtype=np.float64)
    drz_cat = CutoutCatalog(drz, dboxes, src_pos=xy, dtype=np.float64)
    aff = blot.shift_affine(n, x0=float(m), y0=float(m))
    fit, _, _ = find_linear_fit(img_cat, drz_cat, affine=aff, fitgeom='shift', cc_type='ZNCC')
    d = fit['subpixal_img_dxy']
    assert np.all(fit['subpixal_status'] == 0)
    ref64, ref32 = np.zeros((n, 2)), np.zeros((n, 2))
    for k in range(n):
        imct = img_cat[k]
        b = _blots64(drz_cat[k], aff[k:k + 1], imct.data.shape)
        ref64[k] = orc.find_displacement(imct.data, *b, cc_type='ZNCC')
        ref32[k] = orc.find_displacement(imct.data.astype(np.float32).astype(np.float64), *b, cc_type='ZNCC')
    err = np.abs(d - ref64).max(axis=1)
    moved = np.abs(ref32 - ref64).max(axis=1)
    print('float64 catalog vs float64 oracle: max %.2e px; float32-rounded image cutouts move the oracle by '
          'median %.2e, min %.2e px (%d of %d sources >= %.0e)'
          % (err.max(), np.median(moved), moved.min(), np.sum(moved >= 10 * TOL64), n, 10 * TOL64))
    assert err.max() < TOL64
    # the scene discriminates: rounding the image cutouts to float32 moves the oracle's shift by at least 10x the
    # tolerance for most sources (the float32 catalog could not pass the bound above)
    assert np.mean(moved >= 10 * TOL64) >= 0.75


def test_mixed_catalog_dtypes():
    from subpixal_amd import blot
    from subpixal_amd.align import find_linear_fit
    from subpixal_amd.cutout import CutoutCatalog
    img, drz, boxes, xy, wh, t = _branch_scene(np.float64)
    keep = [0, 1, 2, 3]
    img, boxes, xy = img, boxes[keep], xy[keep]
    drz = drz.astype(np.float32).astype(np.float64)                      # float32-representable drizzled values
    m = 8
    dboxes = boxes + np.array([-m, -m, 2 * m, 2 * m], np.int32)
    aff = blot.shift_affine(len(keep), x0=float(m), y0=float(m))

    def run(idt, ddt, dframe=drz, iframe=img):
        ic = CutoutCatalog(iframe, boxes, src_pos=xy + t, dtype=idt)
        dc = CutoutCatalog(dframe, dboxes, src_pos=xy, dtype=ddt)
        fit, iccs, blts = find_linear_fit(ic, dc, affine=aff, fitgeom='shift', cc_type='ZNCC')
        return fit['subpixal_img_dxy'], iccs, blts

    d64, i64, b64 = run(np.float64, np.float64)
    dm, im, bm = run(np.float64, np.float32)
    assert _same_bits(d64, dm)
    assert all(_same_bits(i64[k], im[k]) and _same_bits(b64[k], bm[k]) for k in range(len(keep)))
    # float32 image catalog + float64 drizzled catalog: the float32 result
    drz64 = drz + 1e-9 * np.random.default_rng(3).standard_normal(drz.shape)
    d32, i32, b32 = run(np.float32, np.float32, dframe=drz64.astype(np.float32))
    dx, ix, bx = run(np.float32, np.float64, dframe=drz64)
    assert _same_bits(d32, dx) and i32[0].dtype == np.float32 and bx[0].dtype == np.float32
    assert all(_same_bits(i32[k], ix[k]) and _same_bits(b32[k], bx[k]) for k in range(len(keep)))
    # and the float32 default on float64 frames is the float32 result
    ic = CutoutCatalog(img, boxes, src_pos=xy + t)
    dc = CutoutCatalog(drz64, dboxes, src_pos=xy)
    fit, _, _ = find_linear_fit(ic, dc, affine=aff, fitgeom='shift', cc_type='ZNCC')
    d32b, _, _ = run(np.float32, np.float32, dframe=drz64.astype(np.float32), iframe=img.astype(np.float32))
    assert _same_bits(fit['subpixal_img_dxy'], d32b)


def test_catalog_path_config5_float64_through_find_linear_fit():
    """BASELINE config 5 with float64 frames and catalogs: the bounds of the float32 test and, per source on a
    sample, bit-identity with cc.find_displacement on float64 Cutout objects"""
    import align_catalog
    from subpixal_amd import cc
    out = align_catalog.run(size=4096, nsrc=5000, reps=3, quiet=True, dtype='float64')
    fit, s = out['fit'], out['scene']
    d, st = fit['subpixal_img_dxy'], fit['subpixal_status']
    n = len(s['img_cat'])
    assert n > 4900 and d.shape == (n, 2) and np.all(st[s['compact']] == 0)
    shapes = s['img_cat'].shapes
    pick = np.concatenate([np.arange(8), np.argsort(shapes.max(axis=1))[[0, 1, -1, -2, -40, -60]],
                           np.random.default_rng(1).choice(n, 28, replace=False)])
    for k in pick:
        imct, dzct = s['img_cat'][int(k)], s['drz_cat'][int(k)]
        assert imct.data.dtype == np.float64 and imct.data.shape == tuple(shapes[k])
        b = _blots64(dzct, s['affine'][k:k + 1], imct.data.shape)
        dx, dy, icc, _ = cc.find_displacement(imct.data, b[0], b[1], b[2], b[3], cc_type='NCC', full_output=True)
        assert dx == d[k, 0] and dy == d[k, 1], (k, dx - d[k, 0], dy - d[k, 1])
        assert _same_bits(icc, out['iccs'][int(k)]) and _same_bits(b[0], out['blts'][int(k)])
    print('config 5 float64 via find_linear_fit: warm %.2f ms, median |d - truth| %.3g px, kept %d/%d, offset err %s, '
          'matrix err %.3g' % (1e3 * out['warm_s'], np.median(out['err']), fit['fitmask'].sum(), n,
                               fit['offset'] - out['exact']['offset'],
                               np.abs(fit['fit_matrix'] - out['exact']['fit_matrix']).max()))
    assert np.median(out['err']) < 2e-3
    assert fit['fitmask'].sum() > 4500
    assert np.abs(fit['offset'] - out['exact']['offset']).max() < 1e-3
    assert np.abs(fit['fit_matrix'] - out['exact']['fit_matrix']).max() < 3e-6
