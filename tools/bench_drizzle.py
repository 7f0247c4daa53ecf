#!/usr/bin/env python
"""The drizzle (`resample.DeviceDrizzle`, `spx_drizzle_*`) and one iteration of `align.align_frames` on the scene of
tools/align_catalog.py rendered as K dithered frames: 4096 x 4096, 5000 sources, K = 4, Gaussian noise of sigma
0.002 per frame, a weight map per frame, float32.  Warm, HIP events, median of --reps:

  * `execute()` (all K frames) and one `fast_replace_image` (K - 1 frames);
  * one full `align_frames` iteration, split by stage (host clock around a device synchronisation per stage);
  * beside the kernel, two floors:
      HBM  -- every active frame and its weight read once, sci, wht and ctx written once, at 8 TB/s;
      VALU -- float64 operations per output pixel from a counted census (below) at one operation per lane per
              cycle: 256 CUs x 64 lanes x 2.4 GHz,
    and which of the two binds.

Census for 'square', pixfrac 1, maps near the identity (a 3 x 3 candidate window of which 4 drops overlap the pixel
for a generic sub-pixel offset): per frame 20 operations of set-up (the inverse map of the pixel, the window, the
tile test); per candidate 8 for the drop's centre, 2 to make it pixel-local, 4 for the bounding-box test -- 14 for the
5 candidates that stop there; for the 4 that overlap, 16 more for the corners, 4 edges of 15 (two ordinates, the
clip's compares and selects, the trapezoid), 5 for the sum, its absolute value and the normalisation, 5 for a w, a w d
and the two accumulations: 14 + 86 = 100.  20 + 5 * 14 + 4 * 100 = 490 per pixel and frame.

    python tools/bench_drizzle.py [--size 4096] [--sources 5000] [--frames 4] [--reps 7] [--json out.json]

Needs an MI355X; there is no CPU fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bench_detect import HBM_BYTES_PER_S, event_ms          # noqa: E402

NOISE = 0.002
VALU_OPS_PER_S = 256 * 64 * 2.4e9
OPS_PER_PIXEL_FRAME = 20 + 5 * 14 + 4 * 100


def affine(deg=0.0, scale=1.0, tx=0.0, ty=0.0, about=(0.0, 0.0)):
    """[6] map: rotation by `deg` and `scale` about `about`, which lands on about + (tx, ty)"""
    c, s = scale * np.cos(np.radians(deg)), scale * np.sin(np.radians(deg))
    a = np.array([[c, -s], [s, c]])
    ab = np.asarray(about, np.float64)
    t = ab + (tx, ty) - a @ ab
    return np.array([a[0, 0], a[0, 1], t[0], a[1, 0], a[1, 1], t[1]])


def apply(m, xy):
    xy = np.asarray(xy, np.float64)
    return np.stack([m[0] * xy[..., 0] + m[1] * xy[..., 1] + m[2], m[3] * xy[..., 0] + m[4] * xy[..., 1] + m[5]], axis=-1)


def invert(m):
    a = np.array([[m[0], m[1]], [m[3], m[4]]])
    ai = np.linalg.inv(a)
    t = -ai @ np.array([m[2], m[5]])
    return np.array([ai[0, 0], ai[0, 1], t[0], ai[1, 0], ai[1, 1], t[1]])


def compose(m, g):
    """m o g"""
    a, b = np.array([[m[0], m[1]], [m[3], m[4]]]), np.array([[g[0], g[1]], [g[3], g[4]]])
    ab = a @ b
    t = a @ np.array([g[2], g[5]]) + np.array([m[2], m[5]])
    return np.array([ab[0, 0], ab[0, 1], t[0], ab[1, 0], ab[1, 1], t[1]])


def dither_scene(size=4096, nsrc=5000, nframes=4, seed=5, noise=NOISE, dtype='float32', sigma=4.0, border=80.0):
    """The scene of tools/align_catalog.py (sources on a jittered grid, amplitudes 0.5 .. 2, Gaussians of `sigma`
    px) as `nframes` dithered frames of size x size and the analytically drawn stack on the output grid.

    Frame k sees the sky through its true map T_k (frame pixel -> output pixel): a dither of a few pixels plus a
    fraction, a rotation of some thousandths of a degree about the centre; T_0 is the identity.  A source at output
    position s is drawn at T_k^-1(s).  Every frame has a smooth weight map in 0.75 .. 1.25."""
    rng = np.random.default_rng(seed)
    g = int(np.ceil(np.sqrt(nsrc)))
    cell = (size - 2.0 * border) / g
    cells = rng.choice(g * g, nsrc, replace=False)
    xy = np.stack([border + (cells % g + 0.5) * cell, border + (cells // g + 0.5) * cell], axis=1)
    xy += rng.uniform(-0.17, 0.17, (nsrc, 2)) * cell
    amp = rng.uniform(0.5, 2.0, nsrc)
    c = (size / 2.0, size / 2.0)
    truth = [affine()] + [affine(deg=rng.uniform(-0.004, 0.004), tx=rng.uniform(-4, 4), ty=rng.uniform(-4, 4), about=c)
                          for _ in range(nframes - 1)]
    dtype = np.dtype(dtype)
    half = int(4.5 * sigma)
    gg = np.arange(-half, half + 1)

    def draw(pos):
        f = np.zeros((size, size), dtype)
        for (x, y), a in zip(pos, amp):
            ix, iy = int(round(x)), int(round(y))
            gx = np.exp(-((gg + ix - x) ** 2) / (2 * sigma ** 2))
            gy = np.exp(-((gg + iy - y) ** 2) / (2 * sigma ** 2))
            f[iy - half:iy + half + 1, ix - half:ix + half + 1] += (a * np.outer(gy, gx)).astype(dtype)
        return f

    nrng = np.random.default_rng(seed + 1000)
    frames, weights = [], []
    yy, xx = np.mgrid[0:size, 0:size]
    for k, t in enumerate(truth):
        f = draw(apply(invert(t), xy))
        if noise > 0:
            f += (noise * nrng.standard_normal(f.shape)).astype(dtype)
        frames.append(f)
        weights.append((1.0 + 0.25 * np.sin(xx / (97.0 + 11 * k)) * np.cos(yy / (89.0 + 7 * k))).astype(dtype))
    stack = draw(xy)
    if noise > 0:
        stack += (noise / np.sqrt(max(nframes - 1, 1)) * nrng.standard_normal(stack.shape)).astype(dtype)
    return dict(frames=frames, weights=weights, truth=truth, xy=xy, amp=amp, stack=stack, size=size, noise=noise)


def gauge_free_residual(maps, truth, size):
    """max |M_k(p) - H(T_k(p))| over the frames' corners p, with H the one affine that fits all of them best: what is
    left of the map errors once the freedom to move the whole output grid is taken out"""
    p = np.array([[0.0, 0.0], [size - 1.0, 0.0], [0.0, size - 1.0], [size - 1.0, size - 1.0]])
    src = np.concatenate([apply(t, p) for t in truth])
    dst = np.concatenate([apply(m, p) for m in maps])
    design = np.concatenate([src, np.ones((len(src), 1))], axis=1)
    h, *_ = np.linalg.lstsq(design, dst, rcond=None)
    return float(np.abs(design @ h - dst).max())


def make_catalog(noise):
    from subpixal_amd import catalogs
    return catalogs.DeviceImageCatalog(nsigma=5.0, min_area=5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--sources', type=int, default=5000)
    ap.add_argument('--frames', type=int, default=4)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    import torch
    from subpixal_amd import align, resample
    s = dither_scene(a.size, a.sources, a.frames)
    K, N = a.frames, a.size
    frames = [torch.from_numpy(f).cuda() for f in s['frames']]
    weights = [torch.from_numpy(w).cuda() for w in s['weights']]
    out = dict(size=N, sources=a.sources, frames=K, noise=s['noise'], dtype='float32', reps=a.reps, kernel='square',
               pixfrac=1.0)
    drz = resample.DeviceDrizzle(frames, np.stack(s['truth']), (N, N), weights=weights)
    out['execute_ms'], out['execute_ms_all'] = event_ms(drz.execute, a.reps)
    q = drz.copy()
    q.fast_drop_image(0)
    flip = [0]

    def replace():
        k = flip[0]
        flip[0] = (k + 1) % K
        q.fast_replace_image((k + 1) % K, k)

    out['fast_replace_image_ms'], _ = event_ms(replace, a.reps)
    for kern in ('turbo', 'point'):
        d2 = resample.DeviceDrizzle(frames, np.stack(s['truth']), (N, N), weights=weights, kernel=kern)
        out['execute_%s_ms' % kern], _ = event_ms(d2.execute, a.reps)
    # floors of execute()
    px = float(N) * N
    hbm = (K * 2 * 4 * px + (4 + 4 + 4) * px) / HBM_BYTES_PER_S * 1e3
    valu = K * px * OPS_PER_PIXEL_FRAME / VALU_OPS_PER_S * 1e3
    out.update(hbm_floor_ms=hbm, valu_floor_ms=valu, valu_ops_per_pixel_frame=OPS_PER_PIXEL_FRAME,
               binding_floor='valu' if valu > hbm else 'hbm')
    # one align_frames iteration, by stage (warm: the second of two runs from the same maps)
    stages = None
    for _ in range(2):
        d3 = resample.DeviceDrizzle(frames, np.stack(s['truth']), (N, N), weights=weights)
        stages = {}
        torch.cuda.synchronize()
        fits = align.align_frames(d3, make_catalog(s['noise']), nmax_iter=1, timings=stages, history=True)
    out['align_iteration_ms'] = {k: 1e3 * float(np.sum(v)) for k, v in stages.items()}
    out['align_iteration_calls'] = {k: len(v) for k, v in stages.items()}
    out['align_iteration_total_ms'] = float(sum(out['align_iteration_ms'].values()))
    out['align_sources'] = [int(f['nsources']) for f in fits[0].values()]
    out['align_offsets_px'] = [float(np.linalg.norm(f['offset'])) for f in fits[0].values()]
    print(json.dumps(out))
    if a.json:
        with open(a.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
