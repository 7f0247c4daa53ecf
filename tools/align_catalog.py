#!/usr/bin/env python
"""BASELINE.json config 5 through the API surface the north star keeps: `subpixal_amd.align.find_linear_fit`
on real cutout carriers with VARIABLE shapes (bounding box + padding per source, cutout.py:159-175) and the
reference's 5-image `cc.find_displacement` (align.py:656-699), for a synthetic 4096x4096 frame pair with a
5000-source catalog -- device-resident: the frames live on the GPU, `cutout.CutoutCatalog` describes the
cutouts by a box table, and the whole per-source loop is four kernel launches.

    python tools/align_catalog.py [--size 4096] [--sources 5000] [--dtype float32|float64] [--detect [--noise S]]

--dtype float64 renders both frames in float64 and runs both catalogs in float64 (the reference's semantics for
float64 frames: it computes in the cutouts' dtype).
--detect finds the sources of the drizzled frame on the device (`subpixal_amd.detect.find_sources`: threshold,
labelling, isophotal positions) instead of using the drawn segmentation and the scene's true positions; --noise S
adds Gaussian noise of sigma S to both frames first (default with --detect: 0.002, detection threshold 5 S).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import align_synthetic                                      # noqa: E402  (scene + renderer)


DETECT_NOISE = 0.002         # the faintest source peaks at 0.5 and falls to 0.011 at its segment's edge (2.75 sigma)


def transform(s, xy):
    """the scene's exact drizzled -> image position map"""
    return (xy - s['c']) @ s['f'].T + s['c'] + s['t']


def build(size=4096, nsrc=5000, seed=5, margin=6, pad=3, dtype='float32', noise=0.0, detect=False, min_area=5):
    """Frames, segmentation, catalogs and maps (frames and catalogs in `dtype`).

    Sources sit on a jittered grid (no two closer than ~35 px), 98 % compact (sigma 4 px, segment = ellipse
    with semi-axes of 11..17 px) and 2 % extended (sigma 9..13 px, semi-axes 30..45 px, which swallow
    neighbours).  The drizzled
    frame holds them at xy, the image frame at xy2 = T(xy).  As in the reference, the primary cutouts are the
    segments' bounding boxes + `pad` (cutout.py:138-175; `cutout.primary_cutout_boxes` on the GPU) -- one shape
    per source --, the image cutout of a source is the same box moved by the integer part of the displacement,
    the drizzled cutout is the box grown by `margin`, so the image-cutout -> drizzled-cutout pixel map is a pure
    offset; pixels of a drizzled cutout outside its own segment are masked and zeroed (cutout.py:190,
    align.py:661).

    noise > 0 adds Gaussian noise of that sigma to both frames (its own generator: the scene does not change).
    detect=True: the segmentation, the boxes and the source positions come from `detect.find_sources` on the
    drizzled frame (threshold 5 * noise, or 0.01 without noise; `min_area` pixels at least) and every detected
    position's image-frame counterpart from the scene's exact transform; boxes, maps and catalogs are then
    derived from the detected boxes exactly as from the drawn ones."""
    import torch
    from subpixal_amd import blot, cutout
    rng = np.random.default_rng(seed)
    g = int(np.ceil(np.sqrt(nsrc)))
    cell = (size - 160.0) / g
    cells = rng.choice(g * g, nsrc, replace=False)
    xy = np.stack([80.0 + (cells % g + 0.5) * cell, 80.0 + (cells // g + 0.5) * cell], axis=1)
    xy += rng.uniform(-0.17, 0.17, (nsrc, 2)) * cell
    amp = rng.uniform(0.5, 2.0, nsrc)
    big = rng.random(nsrc) < 0.02
    rx = np.where(big, rng.integers(30, 46, nsrc), rng.integers(11, 18, nsrc))
    ry = np.where(big, rng.integers(30, 46, nsrc), rng.integers(11, 18, nsrc))
    radius = np.maximum(rx, ry)
    sigma = np.where(big, np.minimum(rx, ry) / 3.4, 4.0)
    c = np.array([size / 2.0, size / 2.0])
    th = np.radians(0.002)
    f = 1.00003 * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    f[0, 1] += 1e-5
    t = np.array([0.731, -1.284])
    xy2 = (xy - c) @ f.T + c + t
    dtype = np.dtype(dtype)
    drz_frame = np.zeros((size, size), dtype)
    img_frame = np.zeros((size, size), dtype)
    seg = np.zeros((size, size), np.int32)
    for k in np.argsort(-radius, kind='stable'):              # extended sources first: compact ones on top
        for frame, (x, y) in ((drz_frame, xy[k]), (img_frame, xy2[k])):
            half = int(4.5 * sigma[k])
            gg = np.arange(-half, half + 1)
            ix, iy = int(round(x)), int(round(y))
            gx = np.exp(-((gg + ix - x) ** 2) / (2 * sigma[k] ** 2))
            gy = np.exp(-((gg + iy - y) ** 2) / (2 * sigma[k] ** 2))
            frame[iy - half:iy + half + 1, ix - half:ix + half + 1] += (amp[k] * np.outer(gy, gx)).astype(dtype)
        ax, ay = int(rx[k]), int(ry[k])
        gx, gy = np.arange(-ax, ax + 1), np.arange(-ay, ay + 1)
        ix, iy = int(round(xy[k, 0])), int(round(xy[k, 1]))
        inside = (gy[:, None] / ay) ** 2 + (gx[None, :] / ax) ** 2 <= 1.0
        seg[iy - ay:iy + ay + 1, ix - ax:ix + ax + 1][inside] = k + 1
    if noise > 0:
        nrng = np.random.default_rng(seed + 1000)
        drz_frame += (noise * nrng.standard_normal(drz_frame.shape)).astype(dtype)
        img_frame += (noise * nrng.standard_normal(img_frame.shape)).astype(dtype)
    scene = dict(f=f, t=t, c=c, xy_all=xy, big_all=big, drz_frame=drz_frame, noise=noise)
    drz_d = torch.from_numpy(drz_frame).cuda()
    if detect:
        from subpixal_amd import detect as _detect
        src = _detect.find_sources(drz_d, 5.0 * noise if noise > 0 else 0.01, min_area=min_area)
        seg_d = src.segmentation
        ids, boxes = cutout.primary_cutout_boxes(seg_d, pad=pad)
        ok = (src.flags[ids - 1] & _detect.FLAG_NOFLUX) == 0
        ids, boxes = ids[ok], boxes[ok]
        pos = np.stack([src.x[ids - 1], src.y[ids - 1]], axis=1)
        pos2 = transform(scene, pos)
        weights = None
        compact = src.npix[ids - 1] < 1500                            # (the drawn compact segments hold < 1000 px)
        scene['src'] = src
    else:
        seg_d = torch.from_numpy(seg).cuda()
        ids, boxes = cutout.primary_cutout_boxes(seg_d, pad=pad)        # 8f-3: one pass over the label image
        k = ids - 1                                                      # (a segment can vanish under others)
        pos, pos2 = xy[k], xy2[k]
        weights = rng.uniform(0.5, 2.0, len(k))
        compact = ~big[k]
    shift = np.round(pos2 - pos).astype(np.int32)
    iboxes = boxes.copy()
    iboxes[:, :2] += shift
    dboxes = boxes + np.array([-margin, -margin, 2 * margin, 2 * margin], np.int32)
    img_cat = cutout.CutoutCatalog(torch.from_numpy(img_frame).cuda(), iboxes, src_pos=pos2, src_id=ids,
                                   dtype=dtype)
    drz_cat = cutout.CutoutCatalog(drz_d, dboxes, src_pos=pos, src_weight=weights,
                                   src_id=ids, segmentation_image=seg_d, dtype=dtype)
    img_cat._frame_host, drz_cat._frame_host = img_frame, drz_frame      # (saves the D2H copy when cutouts are built)
    affine = blot.shift_affine(len(ids), x0=(shift[:, 0] + margin).astype(np.float64),
                               y0=(shift[:, 1] + margin).astype(np.float64))
    return dict(img_cat=img_cat, drz_cat=drz_cat, affine=affine, xy=pos, xy2=pos2, compact=compact, **scene)


def run(size=4096, nsrc=5000, reps=5, quiet=False, nclip=12, cc_type='NCC', dtype='float32', noise=0.0,
        detect=False):
    import torch
    from subpixal_amd.align import find_linear_fit, iter_linear_fit
    s = build(size, nsrc, dtype=dtype, noise=noise, detect=detect)
    times = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit, iccs, blts = find_linear_fit(s['img_cat'], s['drz_cat'], affine=s['affine'], fitgeom='general',
                                          nclip=nclip, sigma=3.0, cc_type=cc_type)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    # the transform the fit should find: image positions (1-based) -> drizzled positions, exactly
    exact = iter_linear_fit(s['xy2'] + 1.0, s['xy'] + 1.0, fitgeom='general', nclip=0)
    d = fit['subpixal_img_dxy']
    err = np.abs(d - (s['xy'] - s['xy2'])).max(axis=1)
    out = dict(fit=fit, exact=exact, err=err, first_s=times[0], warm_s=float(np.median(times[1:])),
               scene=s, iccs=iccs, blts=blts)
    nsrc = len(d)
    if not quiet:
        shp = s['img_cat'].shapes
        print('sources %d, frame %dx%d, %d distinct cutout shapes (%d..%d px per side), %s, %s'
              % (nsrc, size, size, len({tuple(x) for x in shp}), shp.min(), shp.max(), cc_type, np.dtype(dtype)))
        print('find_linear_fit(CutoutCatalog, CutoutCatalog): first call %.2f ms, warm %.2f ms (median of %d)'
              % (1e3 * times[0], 1e3 * out['warm_s'], reps))
        print('|shift - truth|: median %.2e, 90%% %.2e px (compact sources: 99%% %.2e); kept %d of %d'
              % (np.median(err), np.percentile(err, 90), np.percentile(err[s['compact']], 99), fit['fitmask'].sum(), nsrc))
        print('offset err %s, matrix err %.2e' % (fit['offset'] - exact['offset'],
                                                   np.abs(fit['fit_matrix'] - exact['fit_matrix']).max()))
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--sources', type=int, default=5000)
    ap.add_argument('--dtype', choices=('float32', 'float64'), default='float32')
    ap.add_argument('--detect', action='store_true', help='sources from detect.find_sources, not the drawn segments')
    ap.add_argument('--noise', type=float, default=None, help='sigma of the noise added to both frames')
    a = ap.parse_args()
    run(a.size, a.sources, dtype=a.dtype, detect=a.detect,
        noise=(DETECT_NOISE if a.detect else 0.0) if a.noise is None else a.noise)
