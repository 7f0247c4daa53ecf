#!/usr/bin/env python
"""`subpixal_amd.detect.find_sources(..., deblend=True)` on the scene of tools/bench_detect.py (4096 x 4096, 5000
sources, Gaussian noise of sigma 0.002, threshold 5 sigma, min_area 5, no filter) with --pairs (default 10 %) of
the compact sources given a companion of 0.6..1.0 times their amplitude 14 px = 3.5 sigma away (sigma 4 px: their isophotes
merge, the deblending tree splits them):

  * find_sources without and with deblend=True, and the deblend entry alone (boxes + spx_deblend_labels_f32),
    warm, HIP events, median of --reps calls;
  * how many parents the deblending split and how many of the drawn pairs came out as two sources;
  * `find_linear_fit` on the drawn-segmentation path of the same scene, the step all of this feeds.

    python tools/bench_deblend.py [--size 4096] [--sources 5000] [--pairs 0.1] [--reps 7] [--json out.json] [--once]

--once: one warm deblending call and nothing else (the process to put under rocprofv3 --kernel-trace --stats).
Needs an MI355X; there is no CPU fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import align_catalog                                        # noqa: E402
from bench_detect import event_ms                           # noqa: E402

PAIR_SEP, PAIR_SIGMA = 14.0, 4.0


def add_pairs(s, share, seed=77):
    """companions for `share` of the compact sources, in a copy of the drizzled frame; returns (frame, [k, x, y])"""
    rng = np.random.default_rng(seed)
    frame = s['drz_frame'].copy()
    compact = np.flatnonzero(~s['big_all'])
    chosen = rng.choice(compact, int(round(share * len(compact))), replace=False)
    comp = []
    half = int(4.5 * PAIR_SIGMA)
    gg = np.arange(-half, half + 1)
    for k in chosen:
        ang = rng.uniform(0, 2 * np.pi)
        x, y = s['xy_all'][k] + PAIR_SEP * np.array([np.cos(ang), np.sin(ang)])
        a = rng.uniform(0.6, 1.0) * float(frame[int(round(s['xy_all'][k, 1])), int(round(s['xy_all'][k, 0]))])
        ix, iy = int(round(x)), int(round(y))
        gx = np.exp(-((gg + ix - x) ** 2) / (2 * PAIR_SIGMA ** 2))
        gy = np.exp(-((gg + iy - y) ** 2) / (2 * PAIR_SIGMA ** 2))
        frame[iy - half:iy + half + 1, ix - half:ix + half + 1] += (a * np.outer(gy, gx)).astype(frame.dtype)
        comp.append((k, x, y))
    return frame, comp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--sources', type=int, default=5000)
    ap.add_argument('--pairs', type=float, default=0.1)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--json', default=None)
    ap.add_argument('--once', action='store_true')
    a = ap.parse_args()
    import torch
    from subpixal_amd import detect
    from subpixal_amd.align import find_linear_fit
    noise, min_area = align_catalog.DETECT_NOISE, 5
    thr = 5.0 * noise
    s = align_catalog.build(a.size, a.sources, noise=noise)
    frame, comp = add_pairs(s, a.pairs)
    fd = torch.from_numpy(frame).cuda()
    labels, n = detect.label(fd, thr, min_area=min_area)
    out_l, n2, parent, dflags = detect.deblend(fd, labels, n, min_area=min_area)
    torch.cuda.synchronize()
    if a.once:
        detect.deblend(fd, labels, n, min_area=min_area)
        torch.cuda.synchronize()
        print('deblend: %d -> %d segments' % (n, n2))
        return
    plain = detect.find_sources(fd, thr, min_area=min_area)
    src = detect.find_sources(fd, thr, min_area=min_area, deblend=True)
    seg = src.segmentation.cpu().numpy()
    seg0 = plain.segmentation.cpu().numpy()
    apart = merged_before = 0
    for k, x, y in comp:
        x0, y0 = s['xy_all'][k]
        p, q = (int(round(y0)), int(round(x0))), (int(round(y)), int(round(x)))
        merged_before += int(seg0[p] == seg0[q] and seg0[p] > 0)
        apart += int(seg[p] != seg[q] and seg[p] > 0 and seg[q] > 0)
    bb = plain.bbox
    box_px = (bb[:, 2] - bb[:, 0] + 1).astype(np.int64) * (bb[:, 3] - bb[:, 1] + 1)
    out = dict(size=a.size, sources=a.sources, pair_share=a.pairs, pairs_drawn=len(comp), pair_sep_px=PAIR_SEP,
               noise=noise, threshold=thr, min_area=min_area, levels=31, contrast=0.005, mode='exponential',
               dtype='float32', reps=a.reps, parents=len(plain), segments=len(src),
               parents_split=int(len(np.unique(src.parent[(src.flags & detect.FLAG_DEBLENDED) != 0]))),
               pairs_merged_before=merged_before, pairs_apart_after=apart,
               parents_one_wave=int((box_px <= 256).sum()), parents_lds=int(((box_px > 256) & (box_px <= 2048)).sum()),
               parents_workspace=int(((box_px > 2048) & (box_px <= 65536)).sum()),
               parents_over_limit=int((box_px > 65536).sum()), median_box_pixels=float(np.median(box_px)))
    out['find_sources_ms'], _ = event_ms(lambda: detect.find_sources(fd, thr, min_area=min_area), a.reps)
    out['find_sources_deblend_ms'], out['find_sources_deblend_ms_all'] = event_ms(
        lambda: detect.find_sources(fd, thr, min_area=min_area, deblend=True), a.reps)
    out['deblend_ms'], out['deblend_ms_all'] = event_ms(lambda: detect.deblend(fd, labels, n, min_area=min_area), a.reps)

    def fit():
        find_linear_fit(s['img_cat'], s['drz_cat'], affine=s['affine'], fitgeom='general', nclip=12, sigma=3.0,
                        cc_type='NCC')
    fit()
    ts = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    out['find_linear_fit_drawn_ms'] = float(np.median(ts))
    print('%dx%d, %d parents (%d one-wave, %d LDS, %d workspace, %d over the limit; median box %d px) -> %d segments; '
          '%d parents split; of %d drawn pairs %d were merged before and %d are apart after'
          % (a.size, a.size, out['parents'], out['parents_one_wave'], out['parents_lds'], out['parents_workspace'],
             out['parents_over_limit'], out['median_box_pixels'], out['segments'], out['parents_split'], len(comp),
             merged_before, apart))
    print('find_sources %.3f ms, with deblend=True %.3f ms; detect.deblend alone %.3f ms; find_linear_fit (drawn '
          'segmentation) %.3f ms' % (out['find_sources_ms'], out['find_sources_deblend_ms'], out['deblend_ms'],
                                    out['find_linear_fit_drawn_ms']))
    print(json.dumps(out))
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
