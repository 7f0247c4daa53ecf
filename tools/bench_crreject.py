#!/usr/bin/env python
"""The cosmic-ray rejection of `resample.DeviceDrizzle(cr_reject=True)` on the scene of tools/bench_drizzle.py
(4096 x 4096, 5000 sources, K = 4, Gaussian noise of sigma 0.002 per frame, a weight map per frame, float32) with
cosmic rays added to every frame: --hits hits of 1 .. 3 pixels per frame, amplitudes 0.3 .. 3.  Warm, HIP events,
median of --reps:

  * the median launch (`spx_drizzle_median_f32`) on its own;
  * the K comparison launches (`spx_drizzle_cr_f32`) on their own, together;
  * the whole `execute()` without and with `cr_reject` (with: packing the rows twice, the median, K comparisons,
    K mask merges, the final drizzle);
  * the share of pixels flagged beside the share drawn.

The median launch is the drizzle's gather with the sums started per frame and a sort in LDS, so it should cost about
one `execute()`; nothing about speed is asserted anywhere.

    python tools/bench_crreject.py [--size 4096] [--sources 5000] [--frames 4] [--hits 20000] [--reps 7] [--json out]

Needs an MI355X; there is no CPU fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bench_detect import event_ms          # noqa: E402
from bench_drizzle import dither_scene      # noqa: E402


def add_hits(frames, rng, nhits, lo=0.3, hi=3.0):
    """`nhits` straight runs of 1 .. 3 pixels per frame; returns the frames and the number of pixels drawn"""
    out, drawn = [], 0
    for f in frames:
        f = f.copy()
        ny, nx = f.shape
        j, i = rng.integers(2, ny - 2, nhits), rng.integers(2, nx - 2, nhits)
        step = np.array([(0, 1), (1, 0), (1, 1), (1, -1)])[rng.integers(0, 4, nhits)]
        length = rng.integers(1, 4, nhits)
        amp = rng.uniform(lo, hi, nhits)
        hit = np.zeros(f.shape, bool)
        for q in range(3):
            on = length > q
            jj, ii = (j + q * step[:, 0])[on], (i + q * step[:, 1])[on]
            np.add.at(f, (jj, ii), (amp[on] * (1.0 if q == 0 else rng.uniform(0.3, 0.9, on.sum()))).astype(f.dtype))
            hit[jj, ii] = True
        out.append(f)
        drawn += int(hit.sum())
    return out, drawn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--sources', type=int, default=5000)
    ap.add_argument('--frames', type=int, default=4)
    ap.add_argument('--hits', type=int, default=20000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    import torch
    from subpixal_amd import _ffi, device, resample
    s = dither_scene(a.size, a.sources, a.frames)
    K, N = a.frames, a.size
    hit_frames, drawn = add_hits(s['frames'], np.random.default_rng(41), a.hits)
    frames = [torch.from_numpy(f).cuda() for f in hit_frames]
    weights = [torch.from_numpy(w).cuda() for w in s['weights']]
    maps = np.stack(s['truth'])
    out = dict(size=N, sources=a.sources, frames=K, hits_per_frame=a.hits, noise=s['noise'], dtype='float32',
               reps=a.reps, kernel='square', pixfrac=1.0)
    plain = resample.DeviceDrizzle(frames, maps, (N, N), weights=weights)
    out['execute_ms'], out['execute_ms_all'] = event_ms(plain.execute, a.reps)
    drz = resample.DeviceDrizzle(frames, maps, (N, N), weights=weights, cr_reject=True, rms=s['noise'])
    out['execute_cr_reject_ms'], out['execute_cr_reject_ms_all'] = event_ms(drz.execute, a.reps)
    flagged = sum(int(m.sum()) for m in drz.output_crmask)
    out.update(drawn_share=drawn / float(K * N * N), flagged_share=flagged / float(K * N * N))
    # the launches on their own, over the rows with the original masks
    lib = _ffi.load()
    rows = torch.from_numpy(drz._pack(drz._order, original=True)).cuda()
    med, nmed = torch.empty_like(drz.output_median), torch.empty_like(drz.output_nmedian)

    def median():
        _ffi.check(lib.spx_drizzle_median_f32(rows.data_ptr(), K, K, 0, 0, 0, N, N, med.data_ptr(), nmed.data_ptr(),
                                              device.stream_ptr()))

    out['median_launch_ms'], out['median_launch_ms_all'] = event_ms(median, a.reps)
    assert torch.equal(med, drz.output_median)
    crm = [torch.empty((N, N), dtype=torch.uint8, device='cuda') for _ in range(K)]
    cln = [torch.empty_like(f) for f in frames]

    def compare():
        for k in range(K):
            _ffi.check(lib.spx_drizzle_cr_f32(rows.data_ptr(), K, k, N, N, med.data_ptr(), nmed.data_ptr(), N, N,
                                              s['noise'], None, 0.0, float('nan'), 3.5, 3.0, 1.2, 0.7,
                                              crm[k].data_ptr(), cln[k].data_ptr(), device.stream_ptr()))

    out['cr_launches_ms'], out['cr_launches_ms_all'] = event_ms(compare, a.reps)
    assert all(torch.equal(x, y) for x, y in zip(crm, drz.output_crmask))
    print(json.dumps(out))
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
