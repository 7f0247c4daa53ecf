"""Times the whole-frame sky statistics (spx_sky_stats_*, csrc/spx_sky_kernels.h) on the K = 4 / 4096 x 4096 scene
of tools/bench_drizzle.py with pedestals of (0, 5, 10, 20) x the noise, and what they replace.

  python tools/bench_sky.py [--size 4096] [--sources 5000] [--out profiles/r15/bench_sky.json]

MEASURED (HIP events around the enqueued call, warm, median of 7): the statistics call for float32 and float64
frames; the same call on constant frames (the tie case: every key equal); `DeviceDrizzle.execute()` without skysub,
the first one with skysub (statistics + subtraction + drizzle) and a later one (frozen values); on the host for ONE
frame: the device -> host copy and the numpy statement (np.median and the clipping loop).

COUNTED from the launch sequence (host::sky_stats_launch): a round reads a frame D + 1 times (D = 3 digit passes for
float32, 6 for float64, one moments pass), and a frame that stops because a round cut nothing has read one more
digit pass; a constant frame reads D passes and no moments.  reads = sum over frames of rounds (D + 1) + (1 if it
stopped that way).  The HBM floor is those bytes at the nominal 8 TB/s; the report gives the call's multiple of it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
HBM_BYTES_PER_S = 8.0e12
PEDESTALS = (0.0, 5.0, 10.0, 20.0)


def timed(fn, reps=7):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def stats_call(frames, clip=5, lsigma=4.0, usigma=4.0):
    """(a closure that enqueues one statistics call, a function that reads its results back)"""
    import torch
    from subpixal_amd import _ffi, device
    lib = _ffi.load()
    K = len(frames)
    dev = frames[0].device
    ft = torch.from_numpy(np.array([f.data_ptr() for f in frames], np.uint64).view(np.int64)).to(dev)
    shapes = torch.from_numpy(np.array([tuple(f.shape) for f in frames], np.int32)).to(dev)
    nbytes = lib.spx_sky_workspace_bytes(K)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty((K, 6), dtype=torch.float64, device=dev)
    counts = torch.empty((K, 2), dtype=torch.int64, device=dev)
    status = torch.empty((K, 2), dtype=torch.int32, device=dev)
    fn = lib.spx_sky_stats_f32 if frames[0].dtype == torch.float32 else lib.spx_sky_stats_f64
    nan = float('nan')

    def call():
        _ffi.check(fn(ft.data_ptr(), None, None, shapes.data_ptr(), K, nan, nan, lsigma, usigma, clip, 0,
                      work.data_ptr(), nbytes, out.data_ptr(), counts.data_ptr(), status.data_ptr(),
                      device.stream_ptr()))
    return call, lambda: (out.cpu().numpy(), counts.cpu().numpy(), status.cpu().numpy())


def reads_of(out, counts, status, digits, clip):
    rounds = status[:, 1]
    const = out[:, 3] == 0
    extra = (~const) & (rounds <= clip)                  # stopped because a round cut nothing: one more digit pass
    per = np.where(const, digits, rounds * (digits + 1) + extra)
    return [int(v) for v in per]


def host_statement(a, clip=5, lsigma=4.0, usigma=4.0):
    v = a[np.isfinite(a)].astype(np.float64)
    lo, hi = -np.inf, np.inf
    for r in range(clip + 1):
        med = np.median(v)
        std = v.std()
        if not std > 0 or r == clip:
            break
        keep = (v >= med - lsigma * std) & (v <= med + usigma * std)
        if keep.all() or not keep.any():
            break
        v = v[keep]
    return float(med)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--sources', type=int, default=5000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r15', 'bench_sky.json'))
    a = ap.parse_args()
    import torch
    import bench_drizzle as bd
    from subpixal_amd import device, resample
    device.init()
    N, K = a.size, 4
    s = bd.dither_scene(N, a.sources, K)
    ped = [np.float32(p * s['noise']) for p in PEDESTALS]
    host = [f + p for f, p in zip(s['frames'], ped)]
    res = dict(size=N, frames=K, sources=a.sources, noise=s['noise'], pedestals=[float(p) for p in ped],
               device=torch.cuda.get_device_name(0), hbm_bytes_per_s_nominal=HBM_BYTES_PER_S)
    for name, tdt, digits in (('float32', torch.float32, 3), ('float64', torch.float64, 6)):
        fr = [torch.from_numpy(f).cuda().to(tdt) for f in host]
        call, read = stats_call(fr)
        ms = timed(call)
        out, counts, status = read()
        reads = reads_of(out, counts, status, digits, 5)
        floor_ms = 1e3 * sum(reads) * N * N * fr[0].element_size() / HBM_BYTES_PER_S
        res[name] = dict(ms=ms, frame_reads=reads, frame_reads_max=6 * (digits + 1), hbm_floor_ms=floor_ms,
                         multiple_of_floor=ms / floor_ms, rounds=status[:, 1].tolist(),
                         sky_minus_pedestal_in_noise=[(out[k, 0] - float(ped[k])) / s['noise'] for k in range(K)])
        const = [torch.full((N, N), 1.5 + k, dtype=tdt, device='cuda') for k in range(K)]
        call, read = stats_call(const)
        cms = timed(call)
        cfloor = 1e3 * K * digits * N * N * const[0].element_size() / HBM_BYTES_PER_S
        res[name + '_constant'] = dict(ms=cms, frame_reads=K * [digits], hbm_floor_ms=cfloor,
                                       multiple_of_floor=cms / cfloor, sky=read()[0][:, 0].tolist())
        del fr, const
    # execute() with and without the subtraction
    maps = np.stack(s['truth'])
    plain = resample.DeviceDrizzle(host, maps, (N, N))
    res['execute_ms'] = timed(plain.execute)

    def first():
        d = resample.DeviceDrizzle([plain._pool[k].data for k in range(K)], maps, (N, N), skysub=True)
        d.execute()
        return d
    first()
    torch.cuda.synchronize()
    t = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d = first()
        torch.cuda.synchronize()
        t.append(1e3 * (time.perf_counter() - t0))
    res['execute_first_with_skysub_wall_ms'] = float(np.median(t))
    res['execute_later_with_skysub_ms'] = timed(d.execute)
    res['computed_sky'] = [d.computed_sky[k] for k in range(K)]
    # the host statement it replaces, one frame
    t0 = time.perf_counter()
    back = plain._pool[3].data.cpu().numpy()
    res['host_copy_one_frame_ms'] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    med = host_statement(back)
    res['host_numpy_one_frame_ms'] = 1e3 * (time.perf_counter() - t0)
    res['host_numpy_sky_frame3'] = med
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == '__main__':
    main()
