#!/usr/bin/env python
"""The error measurements (`spx_measure_errors_*`, `detect.find_sources(..., rms=...)`) on the scene of
tools/bench_detect.py: config 5 of tools/align_catalog.py (4096 x 4096, 5000 sources) with Gaussian noise of sigma
0.002 on the frame, detection threshold 5 sigma, min_area 5, float32, an rms MAP (constant, but read per pixel):

  * find_sources without and with rms=, warm, HIP events, median of --reps calls;
  * the two kernels alone on the same boxes, through the C entries with everything resident: spx_measure_labels_f32
    (the yardstick) and spx_measure_errors_f32;
  * the HBM floor of the new kernel beside it: frame, labels and rms read once over the boxes (12 B per box pixel),
    the measure table's four numbers read and six written per source -- at the 8 TB/s the project's rooflines use.

    python tools/bench_errors.py [--size 4096] [--sources 5000] [--reps 7] [--json out.json] [--once]

--once: one warm find_sources(rms=...) call and nothing else (the process to put under a kernel trace).
Needs an MI355X; there is no CPU fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import align_catalog                                        # noqa: E402
from bench_detect import HBM_BYTES_PER_S, event_ms          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--sources', type=int, default=5000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--json', default=None)
    ap.add_argument('--once', action='store_true')
    a = ap.parse_args()
    import torch
    from subpixal_amd import _ffi, cutout, detect, device
    noise, min_area = align_catalog.DETECT_NOISE, 5
    thr = 5.0 * noise
    s = align_catalog.build(a.size, a.sources, noise=noise)
    fd = torch.from_numpy(s['drz_frame']).cuda()
    rms = torch.full_like(fd, noise)
    src = detect.find_sources(fd, thr, min_area=min_area, rms=rms)
    torch.cuda.synchronize()
    if a.once:
        src = detect.find_sources(fd, thr, min_area=min_area, rms=rms)
        torch.cuda.synchronize()
        print('find_sources(rms=map): %d sources' % len(src))
        return
    n = len(src)
    out = dict(size=a.size, sources=a.sources, noise=noise, threshold=thr, min_area=min_area, detected=n,
               dtype='float32', reps=a.reps)
    out['find_sources_ms'], _ = event_ms(lambda: detect.find_sources(fd, thr, min_area=min_area), a.reps)
    out['find_sources_rms_ms'], _ = event_ms(lambda: detect.find_sources(fd, thr, min_area=min_area, rms=rms), a.reps)
    # the kernels alone: boxes, tables and outputs resident, nothing but the launch inside the events
    lib = _ffi.load()
    seg = src.segmentation
    boxes, _ = cutout.segment_bounding_boxes(seg, max_label=n)
    table = torch.empty((n, 13), dtype=torch.float64, device=fd.device)
    flags = torch.empty((n,), dtype=torch.int32, device=fd.device)
    errors = torch.empty((n, 6), dtype=torch.float64, device=fd.device)
    eflags = torch.empty((n,), dtype=torch.int32, device=fd.device)
    ny, nx = fd.shape
    p = device.ptr

    def measure():
        _ffi.check(lib.spx_measure_labels_f32(p(fd), None, 0.0, None, p(seg), ny, nx, n, p(boxes), p(table), p(flags),
                                              device.stream_ptr()))

    def measure_errors():
        _ffi.check(lib.spx_measure_errors_f32(p(fd), None, 0.0, None, 0.0, p(rms), 0.0, p(seg), ny, nx, n, p(boxes),
                                              p(table), p(errors), p(eflags), device.stream_ptr()))
    out['measure_kernel_ms'], out['measure_kernel_ms_all'] = event_ms(measure, a.reps)
    out['errors_kernel_ms'], out['errors_kernel_ms_all'] = event_ms(measure_errors, a.reps)
    assert torch.equal(table, src.table_device) and torch.equal(errors, src.errors_device)
    out['errors_over_measure'] = out['errors_kernel_ms'] / out['measure_kernel_ms']
    bb = src.bbox.astype(np.int64)
    area = (bb[:, 2] - bb[:, 0] + 1) * (bb[:, 3] - bb[:, 1] + 1)
    box_px = int(area.sum())
    out['box_pixels'], out['box_median'], out['box_max'] = box_px, float(np.median(area)), int(area.max())
    floor = 12 * box_px + n * (4 * 8 + 16 + 6 * 8 + 4)
    out['floor_bytes'] = floor
    out['floor_ms_at_8TBs'] = 1e3 * floor / HBM_BYTES_PER_S
    out['errors_kernel_over_floor'] = out['errors_kernel_ms'] / out['floor_ms_at_8TBs']
    print('find_sources %dx%d, %d sources: %.3f ms warm without rms, %.3f ms with an rms map'
          % (a.size, a.size, n, out['find_sources_ms'], out['find_sources_rms_ms']))
    print('kernels alone over %d boxes (%d px in all, median %d, largest %d): measure %.4f ms, errors %.4f ms (%.2fx)'
          % (n, box_px, out['box_median'], out['box_max'], out['measure_kernel_ms'], out['errors_kernel_ms'],
             out['errors_over_measure']))
    print('HBM floor of the errors kernel %.2f MB = %.5f ms at 8 TB/s: %.0fx the floor'
          % (floor / 1e6, out['floor_ms_at_8TBs'], out['errors_kernel_over_floor']))
    print(json.dumps(out))
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
