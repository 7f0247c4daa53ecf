#!/usr/bin/env python
"""`subpixal_amd.detect.estimate_background` on the scene of tools/bench_detect.py (4096 x 4096, 5000 sources,
Gaussian noise of sigma 0.002), for mesh cells of 64 x 64 and 32 x 32 pixels and float32 and float64 frames:

  * estimate_background warm, HIP events, median of --reps calls, and its two device entries on their own:
    spx_background_mesh_* (bkg_cell_kernel alone: gather, sort and clip of every cell) and spx_background_maps_*
    (bkg_filter_kernel, bkg_global_kernel, bkg_spline_kernel twice -- a few microseconds on a mesh of a few thousand
    nodes -- and bkg_expand_kernel, which writes the maps);
  * the algorithmic HBM floor beside it: the frame read once, the background and rms maps written once (and the
    float32 threshold map where asked for), at the 8 TB/s the project's rooflines use;
  * the host statement (tests/background_statement.py: numpy sort / median / mean / std per cell, scipy CubicSpline)
    on the same frame and this machine's CPU, and the device's agreement with it;
  * find_sources on the same frame, timed the same way: the estimate should cost no more than the detection it feeds.

    python tools/bench_background.py [--size 4096] [--sources 5000] [--reps 7] [--json out.json] [--no-host]

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
import background_statement as bs                           # noqa: E402
from bench_detect import event_ms, HBM_BYTES_PER_S          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--sources', type=int, default=5000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--json', default=None)
    ap.add_argument('--no-host', action='store_true')
    a = ap.parse_args()
    import torch
    from subpixal_amd import _ffi, detect, device
    noise = align_catalog.DETECT_NOISE
    frame32 = align_catalog.build(a.size, a.sources, noise=noise)['drz_frame']
    lib = _ffi.load()
    out = dict(size=a.size, sources=a.sources, noise=noise, reps=a.reps, cases=[])
    fd32 = torch.from_numpy(frame32).cuda()
    out['find_sources_ms'], _ = event_ms(lambda: detect.find_sources(fd32, 5.0 * noise, min_area=5), a.reps)
    for dtype in (np.float32, np.float64):
        fh = frame32.astype(dtype)
        fd = torch.from_numpy(fh).cuda()
        f64 = dtype == np.float64
        for box in ((64, 64), (32, 32)):
            c = dict(dtype=np.dtype(dtype).name, box=list(box))
            c['estimate_background_ms'], c['estimate_background_ms_all'] = event_ms(
                lambda: detect.estimate_background(fd, box=box), a.reps)
            bg = detect.estimate_background(fd, box=box)
            ny, nx = fd.shape
            ncy, ncx = bg.mesh_ngood.shape
            mesh = [torch.empty((ncy, ncx), dtype=torch.float64, device='cuda') for _ in range(2)]
            ng = torch.empty((ncy, ncx), dtype=torch.int32, device='cuda')
            fm = lib.spx_background_mesh_f64 if f64 else lib.spx_background_mesh_f32
            c['mesh_entry_ms'], _ = event_ms(lambda: _ffi.check(fm(
                fd.data_ptr(), None, None, ny, nx, box[0], box[1], 3.0, 10, 0.5, mesh[0].data_ptr(), mesh[1].data_ptr(),
                ng.data_ptr(), device.stream_ptr())), a.reps)
            c['mesh_entry_no_clip_ms'], _ = event_ms(lambda: _ffi.check(fm(
                fd.data_ptr(), None, None, ny, nx, box[0], box[1], 3.0, 0, 0.5, mesh[0].data_ptr(), mesh[1].data_ptr(),
                ng.data_ptr(), device.stream_ptr())), a.reps)
            _ffi.check(fm(fd.data_ptr(), None, None, ny, nx, box[0], box[1], 3.0, 10, 0.5, mesh[0].data_ptr(),
                          mesh[1].data_ptr(), ng.data_ptr(), device.stream_ptr()))
            work = torch.empty(lib.spx_background_workspace_bytes(ny, nx, box[0], box[1]), dtype=torch.uint8, device='cuda')
            maps = [torch.empty_like(fd) for _ in range(2)]
            thr = torch.empty((ny, nx), dtype=torch.float32, device='cuda')
            status = torch.empty(1, dtype=torch.int32, device='cuda')
            fp = lib.spx_background_maps_f64 if f64 else lib.spx_background_maps_f32

            def run_maps(b, r, t):
                _ffi.check(fp(mesh[0].data_ptr(), mesh[1].data_ptr(), ng.data_ptr(), ncy, ncx, box[0], box[1], 3, ny, nx,
                              1.5, work.data_ptr(), work.numel(), b, r, t, status.data_ptr(), device.stream_ptr()))
            c['maps_entry_ms'], _ = event_ms(lambda: run_maps(maps[0].data_ptr(), maps[1].data_ptr(), None), a.reps)
            c['maps_entry_with_threshold_ms'], _ = event_ms(
                lambda: run_maps(maps[0].data_ptr(), maps[1].data_ptr(), thr.data_ptr()), a.reps)
            c['threshold_only_ms'], _ = event_ms(lambda: run_maps(None, None, thr.data_ptr()), a.reps)
            elem = fh.itemsize
            c['floor_bytes'] = 3 * elem * fh.size
            c['floor_ms_at_8TBs'] = 1e3 * c['floor_bytes'] / HBM_BYTES_PER_S
            c['entries_over_floor'] = (c['mesh_entry_ms'] + c['maps_entry_ms']) / c['floor_ms_at_8TBs']
            c['estimate_over_floor'] = c['estimate_background_ms'] / c['floor_ms_at_8TBs']
            c['estimate_over_find_sources'] = c['estimate_background_ms'] / out['find_sources_ms']
            if not a.no_host:
                t0 = time.perf_counter()
                st = bs.statement(fh, box, allow_ties=True)
                c['host_statement_ms'] = 1e3 * (time.perf_counter() - t0)
                c['host_threads_allowed'] = int(os.environ.get('OMP_NUM_THREADS', 0)) or os.cpu_count()
                c['ties_in_scene'] = int(st['mesh']['ties'])
                c['max_abs_bkg_vs_statement'] = float(np.abs(bg.background.cpu().numpy() - st['bkg']).max())
                c['max_abs_rms_vs_statement'] = float(np.abs(bg.rms.cpu().numpy() - st['rms']).max())
            out['cases'].append(c)
            print('%s box %dx%d: estimate_background %.3f ms warm = mesh entry %.3f (%.3f without clipping rounds) + maps '
                  'entry %.3f (+threshold %.3f, threshold alone %.3f) + host; floor %.0f MB = %.3f ms: entries %.1fx, '
                  'call %.1fx; %.2fx find_sources (%.3f ms)%s'
                  % (c['dtype'], box[0], box[1], c['estimate_background_ms'], c['mesh_entry_ms'], c['mesh_entry_no_clip_ms'],
                     c['maps_entry_ms'], c['maps_entry_with_threshold_ms'], c['threshold_only_ms'], c['floor_bytes'] / 1e6,
                     c['floor_ms_at_8TBs'], c['entries_over_floor'], c['estimate_over_floor'],
                     c['estimate_over_find_sources'], out['find_sources_ms'],
                     '' if a.no_host else '; host statement %.0f ms' % c['host_statement_ms']))
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as fh_:
            json.dump(out, fh_, indent=1)


if __name__ == '__main__':
    main()
