#!/usr/bin/env python
"""`subpixal_amd.detect.find_sources` on the config-5 scene of tools/align_catalog.py (4096 x 4096, 5000 sources)
with Gaussian noise of sigma 0.002 on the frames (detection threshold 5 sigma = 0.01, min_area 5, no filter):

  * find_sources and its two halves (label, measure) warm, HIP events, median of --reps calls;
  * the algorithmic HBM floor beside it: the frame read once for the mask and once more over the boxes for the
    measurements, the label image written once and read once (boxes) -- at the 8 TB/s the project's rooflines use;
  * the same mask through scipy.ndimage.label + np.bincount moments on this machine's CPU (the CPU side of the
    line: what a user without the device path runs; neither library threads this work);
  * `find_linear_fit` on the drawn-segmentation path of the same scene, timed the same way, because detection
    must not dominate what it feeds.

    python tools/bench_detect.py [--size 4096] [--sources 5000] [--reps 7] [--json out.json] [--once]

--once: one warm find_sources call and nothing else (the process to put under rocprofv3 --kernel-trace --stats
for the per-kernel split).  Needs an MI355X; there is no CPU fallback."""
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

HBM_BYTES_PER_S = 8e12


def event_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), [float(t) for t in times]


def cpu_statement(frame, thr, min_area):
    """threshold + scipy.ndimage.label + min_area + first moments with numpy, timed"""
    from scipy import ndimage
    t0 = time.perf_counter()
    det = np.isfinite(frame) & (frame > thr)
    lab, n = ndimage.label(det, structure=np.ones((3, 3), int))
    t1 = time.perf_counter()
    area = np.bincount(lab.ravel(), minlength=n + 1)
    keep = area >= min_area
    keep[0] = False
    lab = np.where(keep, np.cumsum(keep), 0).astype(np.int32)[lab]
    sel = lab > 0
    ys, xs = np.nonzero(sel)
    l, w = lab[sel], frame[sel].astype(np.float64)
    flux = np.bincount(l, weights=w)[1:]
    x = np.bincount(l, weights=w * xs)[1:] / flux
    y = np.bincount(l, weights=w * ys)[1:] / flux
    t2 = time.perf_counter()
    return dict(n=int(keep.sum()), mask_label_s=t1 - t0, total_s=t2 - t0), lab, x, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--sources', type=int, default=5000)
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
    frame = s['drz_frame']
    fd = torch.from_numpy(frame).cuda()
    src = detect.find_sources(fd, thr, min_area=min_area)
    torch.cuda.synchronize()
    if a.once:
        src = detect.find_sources(fd, thr, min_area=min_area)
        torch.cuda.synchronize()
        print('find_sources: %d sources' % len(src))
        return
    out = dict(size=a.size, sources=a.sources, noise=noise, threshold=thr, min_area=min_area, detected=len(src),
               dtype='float32', reps=a.reps)
    out['find_sources_ms'], out['find_sources_ms_all'] = event_ms(
        lambda: detect.find_sources(fd, thr, min_area=min_area), a.reps)
    holder = {}

    def lab():
        holder['l'] = detect.label(fd, thr, min_area=min_area)
    out['label_ms'], _ = event_ms(lab, a.reps)
    labels, n = holder['l']
    out['measure_ms'], _ = event_ms(lambda: detect.measure(fd, labels, n), a.reps)
    # the floor: frame once (mask) + label image written once; boxes: label image read once; measurements: frame
    # and labels over the boxes
    npix = frame.size
    box_px = int(((src.bbox[:, 2] - src.bbox[:, 0] + 1).astype(np.int64) * (src.bbox[:, 3] - src.bbox[:, 1] + 1)).sum())
    floor = 4 * npix + 4 * npix + 4 * npix + 8 * box_px
    out['floor_bytes'] = floor
    out['floor_ms_at_8TBs'] = 1e3 * floor / HBM_BYTES_PER_S
    out['time_over_floor'] = out['find_sources_ms'] / out['floor_ms_at_8TBs']
    # bytes the kernels as built move (each pass over a 4-byte frame): tile kernel 3 (frame, L, cnt), compress 3 (L,
    # R, cnt atomics not counted), flag count 2, assign 2, relabel 3 (R, gathered cnt, labels), boxes 1, + boxes' pixels
    out['built_bytes'] = 4 * npix * (3 + 3 + 2 + 2 + 3 + 1) + 8 * box_px
    # the CPU side
    cpu, lab_cpu, x_cpu, y_cpu = cpu_statement(frame, thr, min_area)
    out['cpu_threads_allowed'] = int(os.environ.get('OMP_NUM_THREADS', 0)) or os.cpu_count()
    out['cpu_mask_label_ms'], out['cpu_total_ms'], out['cpu_sources'] = (1e3 * cpu['mask_label_s'],
                                                                         1e3 * cpu['total_s'], cpu['n'])
    out['labels_equal_scipy'] = bool(np.array_equal(lab_cpu, src.segmentation.cpu().numpy()))
    out['max_abs_dxy_vs_numpy'] = float(max(np.nanmax(np.abs(x_cpu - src.x)), np.nanmax(np.abs(y_cpu - src.y))))
    # what it feeds
    def fit():
        find_linear_fit(s['img_cat'], s['drz_cat'], affine=s['affine'], fitgeom='general', nclip=12, sigma=3.0,
                        cc_type='NCC')
    fit()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    out['find_linear_fit_drawn_ms'] = float(np.median(ts))
    # host clock around find_sources as well (it ends in device-to-host copies of the tables)
    ts = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        detect.find_sources(fd, thr, min_area=min_area)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    out['find_sources_host_ms'] = float(np.median(ts))
    print('find_sources %dx%d, %d sources detected: %.3f ms warm (label %.3f, measure %.3f; host clock %.3f ms)'
          % (a.size, a.size, len(src), out['find_sources_ms'], out['label_ms'], out['measure_ms'],
             out['find_sources_host_ms']))
    print('HBM floor %.1f MB = %.3f ms at 8 TB/s: %.1fx the floor (the kernels as built move %.1f MB)'
          % (floor / 1e6, out['floor_ms_at_8TBs'], out['time_over_floor'], out['built_bytes'] / 1e6))
    print('scipy.ndimage.label + numpy moments on the host (%d threads allowed; both libraries run this on one): %.1f '
          'ms (mask + label alone %.1f ms); labels equal: %s, max |x, y - numpy| %.1e px'
          % (out['cpu_threads_allowed'], out['cpu_total_ms'], out['cpu_mask_label_ms'],
                                          out['labels_equal_scipy'], out['max_abs_dxy_vs_numpy']))
    print('find_linear_fit on the drawn segmentation, same scene: %.3f ms warm' % out['find_linear_fit_drawn_ms'])
    print(json.dumps(out))
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
