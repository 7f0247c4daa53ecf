#!/usr/bin/env python
"""minmed and the mask growth of `resample.DeviceDrizzle` on the scene of tools/bench_crreject.py (4096 x 4096, 5000
sources, Gaussian noise of sigma 0.002 per frame, a weight map per frame, float32, 20000 hits per frame), built for
K = 4 frames and, with --use 2, cut to its first two.  Warm, HIP events, median of --reps:

  * the median launch (`spx_drizzle_median_f32`) and, beside it, the minmed entry (`spx_drizzle_minmed_f32`: the gather
    that also tracks the minimum, and the combine_grow stencil pass);
  * the K comparison launches and the K growth launches (`spx_drizzle_cr_grow_f32`, g = 3, c = 16, ctedir = +1), each
    group on its own;
  * the whole `execute()` with `cr_reject` and every new keyword at its default, with 'minmed', and with 'minmed' and
    the growth;
  * the HBM floor of the two stencil passes (every plane read once and written once) at --hbm-gbs.

The two launches inside the minmed entry are told apart by a kernel trace of this script, not here.  Nothing about
speed is asserted anywhere.

    python tools/bench_minmed.py [--size 4096] [--frames 4] [--use 4] [--hits 20000] [--reps 7] [--json out]

Needs an MI355X; there is no CPU fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bench_crreject import add_hits         # noqa: E402
from bench_detect import event_ms           # noqa: E402
from bench_drizzle import dither_scene      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--sources', type=int, default=5000)
    ap.add_argument('--frames', type=int, default=4)
    ap.add_argument('--use', type=int, default=0, help='keep the first USE frames of the scene (0: all)')
    ap.add_argument('--hits', type=int, default=20000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--hbm-gbs', type=float, default=6300.0,
                    help='HBM bandwidth the floors are computed at, GB/s (default: the achievable copy rate)')
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    import torch
    from subpixal_amd import _ffi, device, resample
    s = dither_scene(a.size, a.sources, a.frames)
    K, N = a.use or a.frames, a.size
    hit_frames, drawn = add_hits(s['frames'], np.random.default_rng(41), a.hits)
    frames = [torch.from_numpy(f).cuda() for f in hit_frames[:K]]
    weights = [torch.from_numpy(w).cuda() for w in s['weights'][:K]]
    maps = np.stack(s['truth'])[:K]
    noise = s['noise']
    out = dict(size=N, sources=a.sources, frames=K, scene_frames=a.frames, hits_per_frame=a.hits, noise=noise,
               dtype='float32', reps=a.reps, kernel='square', pixfrac=1.0, hbm_gbs=a.hbm_gbs)
    kw = dict(weights=weights, cr_reject=True, rms=noise)
    drz = resample.DeviceDrizzle(frames, maps, (N, N), **kw)
    out['execute_cr_reject_ms'], out['execute_cr_reject_ms_all'] = event_ms(drz.execute, a.reps)
    mm = resample.DeviceDrizzle(frames, maps, (N, N), combine_type='minmed', **kw)
    out['execute_minmed_ms'], out['execute_minmed_ms_all'] = event_ms(mm.execute, a.reps)
    out['minmed_share'] = float((mm.output_minmed > 0).float().mean())
    out['flagged_share_median'] = sum(int(m.sum()) for m in drz.output_crmask) / float(K * N * N)
    out['flagged_share_minmed'] = sum(int(m.sum()) for m in mm.output_crmask) / float(K * N * N)
    out['drawn_share'] = drawn * K / float(a.frames) / float(K * N * N)
    gr = resample.DeviceDrizzle(frames, maps, (N, N), combine_type='minmed', driz_cr_grow=3, driz_cr_ctegrow=16,
                                driz_cr_ctedir=1, **kw)
    out['execute_minmed_grow_ms'], out['execute_minmed_grow_ms_all'] = event_ms(gr.execute, a.reps)
    out['flagged_share_grown'] = sum(int(m.sum()) for m in gr.output_crmask) / float(K * N * N)
    # the launches on their own, over the rows with the original masks
    lib = _ffi.load()
    rows = torch.from_numpy(drz._pack(drz._order, original=True)).cuda()
    med, nmed = torch.empty_like(drz.output_median), torch.empty_like(drz.output_nmedian)

    def median():
        _ffi.check(lib.spx_drizzle_median_f32(rows.data_ptr(), K, K, 0, 0, 0, N, N, med.data_ptr(), nmed.data_ptr(),
                                              device.stream_ptr()))

    out['median_launch_ms'], out['median_launch_ms_all'] = event_ms(median, a.reps)
    assert torch.equal(med, drz.output_median)
    table = torch.tensor([[noise, 0.0, 0.0]] * K, dtype=torch.float64, device='cuda')
    md, lo = torch.empty_like(med), torch.empty_like(med)
    bits, how = torch.empty_like(nmed), torch.empty_like(nmed)
    med2, nmed2 = torch.empty_like(med), torch.empty_like(nmed)

    def minmed():
        _ffi.check(lib.spx_drizzle_minmed_f32(rows.data_ptr(), K, K, 0, 0, 0, table.data_ptr(), 4.0, 3.0, 1, N, N,
                                              md.data_ptr(), lo.data_ptr(), bits.data_ptr(), med2.data_ptr(),
                                              nmed2.data_ptr(), how.data_ptr(), device.stream_ptr()))

    out['minmed_entry_ms'], out['minmed_entry_ms_all'] = event_ms(minmed, a.reps)
    assert torch.equal(md, med) and torch.equal(med2, mm.output_median) and torch.equal(how, mm.output_minmed)
    out['minmed_over_median'] = out['minmed_entry_ms'] / out['median_launch_ms']
    crm = [torch.empty((N, N), dtype=torch.uint8, device='cuda') for _ in range(K)]
    grown = [torch.empty((N, N), dtype=torch.uint8, device='cuda') for _ in range(K)]
    cln = [torch.empty_like(f) for f in frames]

    def compare():
        for k in range(K):
            _ffi.check(lib.spx_drizzle_cr_f32(rows.data_ptr(), K, k, N, N, med2.data_ptr(), nmed2.data_ptr(), N, N,
                                              noise, None, 0.0, float('nan'), 3.5, 3.0, 1.2, 0.7, crm[k].data_ptr(),
                                              cln[k].data_ptr(), device.stream_ptr()))

    def grow():
        for k in range(K):
            _ffi.check(lib.spx_drizzle_cr_grow_f32(rows.data_ptr(), K, k, N, N, med2.data_ptr(), nmed2.data_ptr(), N, N,
                                                   noise, None, crm[k].data_ptr(), 3, 16, 1, grown[k].data_ptr(),
                                                   cln[k].data_ptr(), device.stream_ptr()))

    out['cr_launches_ms'], out['cr_launches_ms_all'] = event_ms(compare, a.reps)
    out['grow_launches_ms'], out['grow_launches_ms_all'] = event_ms(grow, a.reps)
    assert all(torch.equal(x, y) for x, y in zip(grown, gr.output_crmask))
    # floors: the combine_grow pass reads md, lo (4 bytes each) and the bits and writes med (4) and the plane (1);
    # the growth reads the seed mask and writes the grown one (frame, weight and rms only where a seed is in reach)
    px = float(N) * N
    out['combine_grow_floor_ms'] = 14.0 * px / (a.hbm_gbs * 1e9) * 1e3
    out['grow_floor_ms_per_frame'] = 2.0 * px / (a.hbm_gbs * 1e9) * 1e3
    out['grow_ms_per_frame'] = out['grow_launches_ms'] / K
    out['grow_over_floor'] = out['grow_ms_per_frame'] / out['grow_floor_ms_per_frame']
    print(json.dumps(out))
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
