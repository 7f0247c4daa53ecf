"""The drizzle through polynomial maps (`resample.DeviceDrizzle` with `PolyMap` entries, spx_drizzle_poly_*) and one
iteration of `align.align_frames` on the bench scene of tools/bench_drizzle.py seen through distorted frames: K = 4
float32 frames of 4096 x 4096 with weight maps, 5000 sources, each frame's true map the affine dither composed with
`distortion(size)` -- a radial cubic of +-3 % area change plus a skew-like quadratic term, degree 3 (for the degree-5
rows two small quintic terms more, for degree 1 its linear part).  Warm runs, HIP events, median of 7:

  * `execute()` for degree 1, 3 and 5 with 'square'; degree 3 with 'turbo' and 'point'; pixfrac 1 and 0.6;
  * one `fast_replace_image` (K - 1 frames), as tools/bench_drizzle.py times it;
  * one `align_frames` iteration by stage (host clock around a device synchronisation per stage);
  * the AFFINE `execute()` on the undistorted scene with this build and, with --parent-lib, with another build of the
    library (the parent commit's), in alternating child processes; this build's median must lie inside the other's
    own min .. max over its repeats;
  * the kernel's two floors, as tools/bench_drizzle.py states them: HBM (frames and weights read once, sci, wht, ctx
    written once, at 8 TB/s) and float64 VALU (one operation per lane per cycle on 256 CUs x 64 lanes x 2.4 GHz).

Census for 'square', pixfrac 1, degree D, a map near the identity (a 3 x 3 candidate window of which 4 drops overlap
the pixel), E = 2 * D (D + 3) / 2 = D (D + 3) operations per evaluated coordinate (multiply and add counted apart:
contraction is off):
  per frame   20 for the linear estimate, the window and the tile test; per chord step 2 E + 12 (two coordinates,
              the residual, A^-1 times it, the update), `steps` of them (3 on this scene);
  per row     of 3 candidates: 4 + 2 + 2 corners = 16 coordinates (the left corners are the neighbour's right
              ones), each E + 1 (pixel-local), so 3 rows x 16 x (E + 1);
  per candidate 6 for (u, v) and the four half-drop offsets, 16 for the bounding box and its test: 9 x 22;
  per overlapping candidate 4 edges of 30 (ends ordered, dx, dy, a division counted as 10 at each kind of crossing
              that occurs -- on average one per edge --, the clip's compares and selects, the trapezoid), 4 for the
              sum and its absolute value, 8 for area(Q), 10 for the quotient, 5 for a w, a w d and the two sums: 147.
  D = 3 (E = 18): 20 + 3 x 48 + 48 x 19 + 198 + 4 x 147 = 1862 per pixel and frame (the affine kernel: 490).

    python tools/bench_drizzle_poly.py [--size 4096] [--sources 5000] [--parent-lib PATH] [--out FILE]

Needs an MI355X; there is no CPU fallback."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def _slot(i, j):
    return (i + j) * (i + j + 1) // 2 + j


def distortion(size, degree=3, dx=0.0, dy=0.0):
    """identity + k r^2 (u, v) + q (u v, -u v / 2) about the frame's centre, k so that the area factor 1 + 4 k r^2
    runs over +-3 % between the centre and the corners, shifted by the dither (dx, dy)"""
    from subpixal_amd.resample import PolyMap
    c = 0.5 * (size - 1)
    k = 0.06 / (4.0 * 2.0 * c * c)
    q = 2e-3 / size
    coef = np.zeros((2, 21))
    coef[0, 0], coef[1, 0] = c + dx, c + dy
    coef[0, 1] = coef[1, 2] = 1.0 - 0.03 / 2                      # -3 % at the centre, +3 % at the corners
    if degree >= 2:
        coef[0, _slot(1, 1)], coef[1, _slot(1, 1)] = q, -0.5 * q
    if degree >= 3:
        coef[0, _slot(3, 0)] = coef[0, _slot(1, 2)] = coef[1, _slot(2, 1)] = coef[1, _slot(0, 3)] = k
    if degree >= 5:
        coef[0, _slot(5, 0)] = coef[1, _slot(0, 5)] = 1e-3 / c ** 4
    return PolyMap(coef, degree, (c, c))


def as_callable(m):
    """a [6] map or a PolyMap as (x, y) -> (X, Y)"""
    if callable(m):
        return m
    m = np.asarray(m, np.float64)
    return lambda x, y: (m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5])


def gauge_free_residual(maps, truth, size):
    """`bench_drizzle.gauge_free_residual` for callables: max |M_k(p) - H(T_k(p))| over a 5 x 5 lattice of frame
    positions p (corners included), with H the one affine that fits all frames best -- what is left of the map errors
    once the freedom to move the whole output grid is taken out"""
    g = np.linspace(0.0, size - 1.0, 5)
    px, py = [v.ravel() for v in np.meshgrid(g, g)]
    src = np.concatenate([np.stack(as_callable(t)(px, py), axis=1) for t in truth])
    dst = np.concatenate([np.stack(as_callable(m)(px, py), axis=1) for m in maps])
    design = np.concatenate([src, np.ones((len(src), 1))], axis=1)
    h, *_ = np.linalg.lstsq(design, dst, rcond=None)
    return float(np.abs(design @ h - dst).max())


def distorted_scene(size=384, nsrc=81, nframes=4, seed=7, sigma=2.5, border=30.0, noise=0.002, dtype='float32'):
    """The scene of `bench_drizzle.dither_scene` seen through distorted frames: frame k's true map is the degree-3
    `PolyMap` T_k = distortion(size) o G_k, G_k the affine dither of that scene (G_0 the identity).  A source at output
    position s is drawn into frame k at T_k^-1(s) with its amplitude as it is -- surface brightness, no Jacobian
    factor, matching "sci is a weighted mean of input values" (the source's shape is not distorted: at 3 % over the
    frame that changes a sigma of 2.5 px by under 0.04 px and moves no centre).  Returns the frames, the same frames
    without noise (`clean`), each frame's noise field, the noise-free stack drawn on the output grid, the truth."""
    import bench_drizzle as bd
    rng = np.random.default_rng(seed)
    g = int(np.ceil(np.sqrt(nsrc)))
    cell = (size - 2.0 * border) / g
    cells = rng.choice(g * g, nsrc, replace=False)
    xy = np.stack([border + (cells % g + 0.5) * cell, border + (cells // g + 0.5) * cell], axis=1)
    xy += rng.uniform(-0.17, 0.17, (nsrc, 2)) * cell
    amp = rng.uniform(0.5, 2.0, nsrc)
    c = (size / 2.0, size / 2.0)
    dith = [bd.affine()] + [bd.affine(deg=rng.uniform(-0.004, 0.004), tx=rng.uniform(-4, 4), ty=rng.uniform(-4, 4),
                                      about=c) for _ in range(nframes - 1)]
    base = distortion(size, 3)
    # (the distortion shrinks the centre by 1.5 %: scaled back so that the frame covers the output grid)
    truth = [base.compose(bd.compose(bd.affine(scale=1.0 / 0.985, about=c), d)) for d in dith]
    dtype = np.dtype(dtype)
    half = int(4.5 * sigma)
    gg = np.arange(-half, half + 1)

    def draw(pos):
        f = np.zeros((size, size), dtype)
        for (x, y), a in zip(pos, amp):
            ix, iy = int(round(x)), int(round(y))
            if not (half <= ix < size - half and half <= iy < size - half):
                continue
            gx = np.exp(-((gg + ix - x) ** 2) / (2 * sigma ** 2))
            gy = np.exp(-((gg + iy - y) ** 2) / (2 * sigma ** 2))
            f[iy - half:iy + half + 1, ix - half:ix + half + 1] += (a * np.outer(gy, gx)).astype(dtype)
        return f

    nrng = np.random.default_rng(seed + 1000)
    clean = [draw(np.stack(t.inverse(xy[:, 0], xy[:, 1]), axis=1)) for t in truth]
    fields = [(noise * nrng.standard_normal((size, size))).astype(dtype) for _ in truth]
    return dict(frames=[f + n for f, n in zip(clean, fields)], clean=clean, noise_fields=fields, truth=truth, xy=xy,
                amp=amp, drawn=draw(xy), size=size, noise=noise)


def timed(fn, reps=7):
    import torch
    fn()
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
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))


def census(D, steps):
    E = D * (D + 3)
    return 20 + steps * (2 * E + 12) + 48 * (E + 1) + 9 * 22 + 4 * 147


def affine_only(size, nsrc, reps):
    """the affine execute() on the undistorted bench scene: one JSON line (run in a child process per library)"""
    import torch
    import bench_drizzle as bd
    from subpixal_amd import _ffi, resample
    if os.environ.get('SPX_HIP_LIB'):                   # an older build has no polynomial entries: not needed here
        for name in [k for k in _ffi._SIGNATURES if k.startswith('spx_drizzle_poly')]:
            del _ffi._SIGNATURES[name]
    s = bd.dither_scene(size, nsrc, 4)
    frames = [torch.from_numpy(f).cuda() for f in s['frames']]
    weights = [torch.from_numpy(w).cuda() for w in s['weights']]
    d = resample.DeviceDrizzle(frames, np.stack(s['truth']), (size, size), weights=weights)
    print(json.dumps(timed(d.execute, reps)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4096)
    ap.add_argument('--sources', type=int, default=5000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--parent-lib', default=None, help='another build of libsubpixal_hip.so for the affine A/B')
    ap.add_argument('--affine-only', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.affine_only:
        return affine_only(args.size, args.sources, args.reps)
    import subprocess
    import torch
    import bench_drizzle as bd
    from bench_detect import HBM_BYTES_PER_S
    from subpixal_amd import _ffi, align, resample
    n, K = args.size, 4
    s = distorted_scene(n, args.sources, K, seed=5, sigma=4.0, border=80.0, noise=bd.NOISE)
    frames = [torch.from_numpy(f).cuda() for f in s['frames']]
    yy, xx = np.mgrid[0:n, 0:n]
    weights = [torch.from_numpy((1.0 + 0.25 * np.sin(xx / (97.0 + 11 * k)) * np.cos(yy / (89.0 + 7 * k))).astype(np.float32)).cuda()
               for k in range(K)]
    del yy, xx
    out = dict(size=n, sources=args.sources, frames=K, dtype='float32', reps=args.reps, results={})

    def run(label, maps, **kw):
        d = resample.DeviceDrizzle(frames, maps, (n, n), weights=weights, **kw)
        d.execute()
        r = timed(d.execute, args.reps)
        if any(isinstance(m, resample.PolyMap) for m in maps):
            w, g = _ffi.DRIZZLE_POLY_ROW_WINDOW, _ffi.DRIZZLE_POLY_ROW_DEGREE
            r['window'] = [float(v) for v in d._rows_host[1, w:w + 16].view(np.float64)]
            r['steps'] = int(d._rows_host[1, g:g + 8].view(np.int32)[1])
        r['covered'] = float((d.output_wht > 0).float().mean())
        out['results'][label] = r
        print('%-36s median %.3f ms (min %.3f max %.3f)' % (label, r['median_ms'], r['min_ms'], r['max_ms']), flush=True)
        return d

    truth3 = s['truth']
    # the same frames' maps cut down to degree 1 (their linear part) and raised to degree 5 (two small quintic terms)
    lin = [resample.PolyMap(m.about((0.5 * (n - 1), 0.5 * (n - 1))).coef, 1, (0.5 * (n - 1), 0.5 * (n - 1))) for m in truth3]
    c5 = []
    for m in truth3:
        m0 = m.about((0.5 * (n - 1), 0.5 * (n - 1)))
        c = m0.coef.copy()
        c[0, _slot(5, 0)] = c[1, _slot(0, 5)] = 1e-3 / (0.5 * n) ** 4
        c5.append(resample.PolyMap(c, 5, m0.center))
    run('poly degree 1 square p=1', lin)
    d3 = run('poly degree 3 square p=1', truth3)
    run('poly degree 5 square p=1', c5)
    run('poly degree 3 square p=0.6', truth3, pixfrac=0.6)
    run('poly degree 3 turbo p=1', truth3, kernel='turbo')
    run('poly degree 3 point', truth3, kernel='point')
    q = d3.copy()
    q.fast_drop_image(0)
    flip = [0]

    def replace():
        k = flip[0]
        flip[0] = (k + 1) % K
        q.fast_replace_image((k + 1) % K, k)
    r = timed(replace, args.reps)
    out['results']['poly degree 3 fast_replace_image'] = r
    print('%-36s median %.3f ms (min %.3f max %.3f)' % ('one fast_replace_image (3 frames)', r['median_ms'], r['min_ms'], r['max_ms']))
    # floors of execute(), degree 3
    steps = out['results']['poly degree 3 square p=1']['steps']
    px = float(n) * n
    hbm = (K * 2 * 4 * px + (4 + 4 + 4) * px) / HBM_BYTES_PER_S * 1e3
    for D, label in ((1, 'poly degree 1 square p=1'), (3, 'poly degree 3 square p=1'), (5, 'poly degree 5 square p=1')):
        st = out['results'][label]['steps']
        ops = census(D, st)
        valu = K * px * ops / bd.VALU_OPS_PER_S * 1e3
        out['results'][label].update(valu_ops_per_pixel_frame=ops, valu_floor_ms=valu, hbm_floor_ms=hbm,
                                     binding_floor='valu' if valu > hbm else 'hbm',
                                     times_floor=out['results'][label]['median_ms'] / max(valu, hbm))
        print('degree %d: %d operations per pixel and frame, VALU floor %.3f ms, HBM floor %.3f ms: %s bound, at %.2fx'
              % (D, ops, valu, hbm, out['results'][label]['binding_floor'], out['results'][label]['times_floor']))
    # one align_frames iteration by stage (warm: the second of two runs from the same maps)
    stages = None
    for _ in range(2):
        d = resample.DeviceDrizzle(frames, truth3, (n, n), weights=weights)
        stages = {}
        torch.cuda.synchronize()
        fits = align.align_frames(d, bd.make_catalog(s['noise']), nmax_iter=1, timings=stages, history=True)
    out['align_iteration_ms'] = {k: 1e3 * float(np.sum(v)) for k, v in stages.items()}
    out['align_iteration_total_ms'] = float(sum(out['align_iteration_ms'].values()))
    out['align_sources'] = [int(f['nsources']) for f in fits[0].values()]
    out['align_offsets_px'] = [float(np.linalg.norm(f['offset'])) for f in fits[0].values()]
    print('align_frames iteration %.1f ms: %s; sources %s; offsets px %s' % (
        out['align_iteration_total_ms'], ' '.join('%s %.1f' % kv for kv in out['align_iteration_ms'].items()),
        out['align_sources'], ' '.join('%.1e' % v for v in out['align_offsets_px'])), flush=True)
    del frames, weights, d, d3, q
    torch.cuda.empty_cache()
    # the affine execute() with this build and with the other library, alternating fresh child processes
    ab = {'this': [], 'parent': []}
    libs = [('this', None)] + ([('parent', os.path.abspath(args.parent_lib))] if args.parent_lib else [])
    for rnd in range(3):
        for name, lib in libs:
            env = dict(os.environ)
            env.pop('SPX_HIP_LIB', None)
            if lib:
                env['SPX_HIP_LIB'] = lib
            txt = subprocess.check_output([sys.executable, os.path.abspath(__file__), '--affine-only', '--size', str(n),
                                           '--sources', str(args.sources), '--reps', str(args.reps)], env=env,
                                          universal_newlines=True, timeout=300)
            ab[name].append(json.loads(txt.strip().splitlines()[-1]))
            print('affine execute(), %s build, round %d: median %.3f ms (min %.3f max %.3f)'
                  % (name, rnd, ab[name][-1]['median_ms'], ab[name][-1]['min_ms'], ab[name][-1]['max_ms']), flush=True)
    out['affine_ab'] = ab
    if ab['parent']:
        med = float(np.median([r['median_ms'] for r in ab['this']]))
        lo, hi = min(r['min_ms'] for r in ab['parent']), max(r['max_ms'] for r in ab['parent'])
        out['affine_unchanged'] = bool(lo <= med <= hi)
        print('affine path: this build median %.3f ms, parent min .. max %.3f .. %.3f ms: %s'
              % (med, lo, hi, 'inside' if out['affine_unchanged'] else 'OUTSIDE'))
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
