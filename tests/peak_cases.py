"""Pair mode and reference mode with the correlation peak anywhere in the lag window: the cases, the backends and
the checks that tests/test_peak_window_cpu.py (CPU threads, tests/emu.py) and tests/test_gpu_peak_window.py
(the device, subpixal_amd) share.

Every kernel family places its refinement window around the coarse arg-max and reads the correlation circularly
from there; the index arithmetic changes form where that window crosses the period (or the class plane).  Which
form runs depends on the peak through conv_index(n, q) = (n-1-q) + (n-1)//2: a source displaced by t px has its
coarse peak at q = (n-1)//2 + round(t), convolution index l_c = n - 1 - round(t).  The shifts below sweep t over
everything a spot that fits its cutout allows, and `window_classes` -- a Python mirror of each family's window
arithmetic, read off the kernel source -- says which forms a case list reaches.

The reference is the float64 oracle (oracle/subpixal_oracle.py), not the drawn shift: at these positions the spot
is cut off by the cutout edge and the oracle itself is up to 8e-2 px from the drawn shift.

Ties are left out.  A shift t with t * U half-way between two integers puts two samples of the fine grid at the
same height in exact arithmetic; float32 and float64 pick different ones and the 5x5 fit box moves by a sample
(measured 2e-3 .. 4e-2 px at upsample 1 and t = +-0.5, symmetric about the tie).  That is the input, not the
kernel: `shifts` drops every t with |frac(t U) - 0.5| < 0.1 at the upsample U it would be used with, and
`assert_no_ties` proves it on the case list.  No case is left out by its status: the oracle's status is 0 for every
pair here, and the checks require 0 on both sides."""
import functools
import os
import subprocess
import sys

import numpy as np

import datagen
from oracle import subpixal_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---------------------------------------------------------------------------------------------------------------
# the kernel families (spx_capi.hip tile_for / run_pair_*): name -> shapes (ny, nx), upsamples, refine forms, the
# `tile=` that forces the family on the CPU harness.  Shapes: the smallest that still reach the family's window
# classes (see window_classes), a full tile, and ragged ones with the long side on either axis.
# ---------------------------------------------------------------------------------------------------------------
FAMILIES = {
    'tile32': dict(tile=32, shapes=((20, 20), (32, 32), (12, 31)), ups=(1, 2, 10, 27), refines=('default',)),
    'tile64': dict(tile=64, shapes=((33, 33), (40, 40), (64, 64), (64, 37), (37, 64)), ups=(1, 2, 10, 27),
                   refines=('float32', 'float64')),
    # SPX_PAIR64_WAVES=8 (spx_kernels8.h): float32 refine only
    'wave8': dict(tile=648, shapes=((33, 33), (40, 40), (64, 64), (64, 37), (37, 64)), ups=(1, 2, 10, 27),
                  refines=('float32',)),
    'fold': dict(tile=64, shapes=((65, 65), (80, 80), (85, 85), (85, 20), (20, 85)), ups=(1, 2, 10, 27),
                 refines=('float32', 'float64')),
    'p192': dict(tile=192, shapes=((86, 86), (96, 96), (100, 100), (128, 128), (128, 70)), ups=(1, 2, 10, 27),
                 refines=('default',)),
    # class count C = big_class_count: 129 px -> 4 (even), 200 px -> 5 (odd), 30x260 -> 7
    'general': dict(tile=0, shapes=((129, 129), (200, 200), (30, 260)), ups=(1, 10, 27), refines=('default',)),
}
CC_TYPES = ('CC', 'ZNCC')
ALL_UPS = (1, 2, 10, 27)


def conv_index(n, q):
    return (n - 1 - q) + (n - 1) // 2


def big_class_count(ny, nx):
    """spx_kernels_big.h big_class_count: the smallest C whose period 64 C keeps the 'same' window alias free"""
    n = max(ny, nx)
    return (2 * n - 2 - (n - 1) // 2 + 1 + 63) // 64


def sigma_for(ny, nx):
    """a spot that fits its cutout (sigma <= min(6 px, side / 6)) and leaves the sweep room:
    2, 3, 4 px up to 24, 36, 48 px of the short side, 5 px up to 128 px, 6 px above"""
    side = min(ny, nx)
    return 2.0 if side <= 24 else 3.0 if side <= 36 else 4.0 if side <= 48 else 5.0 if side <= 128 else 6.0


def shift_limit(n, sigma):
    """the spot's centre stays 2.2 sigma inside both cutouts (the reference has it at (n-1)/2), and the two spots
    overlap: a float32 spot is exactly 0 beyond 14.4 sigma, and where the image's non-zero pixels see only zeros of
    the reference the reference's own NCC / ZNCC is 0 / 0 (cc.py:131-156) -- only 30x260 gets that far"""
    return min((n - 1) / 2.0 - 2.2 * sigma, 20.0 * sigma)


EXTRA_SHIFTS = (-2.5, -0.5, 0.5, 1.5, 2.49)      # sub-pixel positions around the centre


def is_tie(t, up):
    x = t * up
    return abs(abs(x - np.floor(x)) - 0.5) < 0.1


def _axis_sweep(n, sigma):
    """nine whole pixels from one end of what fits to the other, each plus 0.37: frac(0.37 U) = .37, .74, .70, .99
    at upsample 1, 2, 10, 27 -- no tie at any of them"""
    lim = shift_limit(n, sigma)
    lo, hi = -int(np.floor(lim + 0.37)), int(np.floor(lim - 0.37))
    return [float(v) + 0.37 for v in np.round(np.linspace(lo, hi, 9))]


def shifts(ny, nx, up):
    """[(tx, ty)] of one cell.  ty walks its list in the opposite direction to tx, so that both axes see both
    ends; a pair is left out at this upsample if either of its shifts is a tie there."""
    sg = sigma_for(ny, nx)
    lim = min(shift_limit(ny, sg), shift_limit(nx, sg))
    extra = [t for t in EXTRA_SHIFTS if abs(t) <= lim]
    sx = _axis_sweep(nx, sg) + extra
    sy = _axis_sweep(ny, sg)[::-1] + extra[::-1]
    return [(tx, ty) for tx, ty in zip(sx, sy) if not (is_tie(tx, up) or is_tie(ty, up))]


def assert_no_ties():
    count = 0
    for fam in FAMILIES.values():
        for ny, nx in fam['shapes']:
            sg = sigma_for(ny, nx)
            assert sg <= min(6.0, min(ny, nx) / 6.0), (ny, nx, sg)
            for up in fam['ups']:
                cell = shifts(ny, nx, up)
                assert len(cell) >= 9, (ny, nx, up, len(cell))        # the whole sweep survives at every upsample
                for tx, ty in cell:
                    for t, n in ((tx, nx), (ty, ny)):
                        assert abs(abs(t * up - np.floor(t * up)) - 0.5) >= 0.1, (ny, nx, up, t)
                        assert abs(t) <= shift_limit(n, sg) + 1e-9, (ny, nx, t)
                    count += 1
            for t in (0.5, -0.5):       # +-0.5 stays exactly where t U is an integer
                kept = [up for up in fam['ups'] if any(tx == t for tx, _ in shifts(ny, nx, up))]
                assert kept == [up for up in fam['ups'] if up % 2 == 0 and shift_limit(min(ny, nx), sg) >= 0.5]
    return count


@functools.lru_cache(maxsize=None)
def pairs(ny, nx, up, dtype='float32'):
    sg = sigma_for(ny, nx)
    prs = [datagen.pair_set(ny, nx, tx, ty, sg, amp=1.3, dtype=np.dtype(dtype)) for tx, ty in shifts(ny, nx, up)]
    ref, img = np.stack([p[0] for p in prs]), np.stack([p[1] for p in prs])
    ref.setflags(write=False)
    img.setflags(write=False)
    return ref, img


@functools.lru_cache(maxsize=None)
def oracle_pairs(ny, nx, up, cc, sel):
    """the float64 definition, once per cell (pairs `sel` of it): every refine form and both 64-tile kernels share it"""
    ref, img = pairs(ny, nx, up)
    exp, est = orc.xcorr_refine_batch(ref[list(sel)], img[list(sel)], up, cc)
    exp.setflags(write=False)
    return exp, est


# ---------------------------------------------------------------------------------------------------------------
# Python mirror of the window arithmetic, per family.  For a peak at flipped index q on an axis of n pixels (the
# cutout's other side is m: the tile is chosen by max(n, m)):
#   32 tile   (spx_kernels32.h fine_window32): class planes of 32, rows m = l_c + k - 16, k in [0, 32), read at
#             m & 31 with the odd class negated where (m >> 5) & 1
#   64 tile   (spx_kernels.h fine_window / fine_window_rolled, spx_kernels8.h fine_window8): planes of 64, rows
#             m = l_c + k - 32, k in [0, 64), read at m & 63, odd class negated where (m >> 6) & 1; the rolled form
#             keeps d0 = l_c - 32 as table offset d0 & 63 and flip (d0 >> 6) & 1
#   period 192 (spx_kernels128.h fine_window128): the whole period, rows wrap(l_c + k - 96); per lane 3 columns
#             from col0 = wrap(l_c + 48 w + 3 lj - 96) in one load, which runs into the wrap-copy columns P, P+1
#             of the row for col0 = P-2 (one) or P-1 (two): some lane has that iff l_c % 3 = 1 or 2 (x axis)
#   general   (spx_kernels_big.h fine_window_big): the whole period P = 64 C, G.wrap(l_c + k - P/2)
# and for the coarse stage of the 64 tile (coarse_argmax, spx_kernels8.h 529-549): plane index mx = l & 63 stands
# for l = mx + 64 where `wrap = mx < lox`, lox = (n-1)//2, with the odd class negated there.
# ---------------------------------------------------------------------------------------------------------------
def family_of(ny, nx):
    n = max(ny, nx)
    return 'tile32' if n <= 32 else 'tile64' if n <= 64 else 'fold' if n <= 85 else 'p192' if n <= 128 else 'general'


def window_geometry(family, ny, nx):
    """(block, half): the unit the window start is counted in, and the distance from l_c to the window start"""
    if family == 'tile32':
        return 32, 16
    if family in ('tile64', 'wave8', 'fold'):
        return 64, 32
    p = 192 if family == 'p192' else 64 * big_class_count(ny, nx)
    return p, p // 2


def window_class(family, ny, nx, axis, q):
    """what the family's index arithmetic depends on, for a window centred on flipped index q of `axis` (0: y)"""
    n = (ny, nx)[axis]
    block, half = window_geometry(family, ny, nx)
    lc = conv_index(n, q)
    d0 = lc - half
    cls = {'start': d0 // block}                 # -1: below 0; 0: inside the first plane / period; 1: past it
    if family in ('tile64', 'wave8', 'fold'):
        cls['flip'] = (d0 >> 6) & 1              # sign of the odd class at the window start
        cls['coarse_wrap'] = int((lc & 63) < (n - 1) // 2)
    if family == 'tile32':
        cls['flip'] = (d0 >> 5) & 1
        cls['coarse_wrap'] = int((lc & 31) < (n - 1) // 2)
    if family == 'p192' and axis == 1:
        cls['wrap_copy_columns'] = lc % 3
    return cls


def reachable_classes(family, ny, nx, axis):
    """the classes of every peak position a spot that fits the cutout can have"""
    n = (ny, nx)[axis]
    lim = shift_limit(n, sigma_for(ny, nx))
    out = {}
    for t in range(-int(np.floor(lim + 0.37)), int(np.floor(lim - 0.37)) + 2):
        for k, v in window_class(family, ny, nx, axis, (n - 1) // 2 + t).items():
            out.setdefault(k, set()).add(v)
    return out


def reached_classes(family, axis):
    """(reached, reachable) over the family's case list: the coarse peak of a pair is the sample next to its shift"""
    got, can = {}, {}
    for ny, nx in FAMILIES[family]['shapes']:
        n = (ny, nx)[axis]
        for k, v in reachable_classes(family, ny, nx, axis).items():
            can.setdefault(k, set()).update(v)
        for up in FAMILIES[family]['ups']:
            for pr in shifts(ny, nx, up):
                q = (n - 1) // 2 + int(np.floor(pr[1 - axis] + 0.5))
                for k, v in window_class(family, ny, nx, axis, q).items():
                    got.setdefault(k, set()).add(v)
    return got, can


# what each family must reach on BOTH axes.  Not listed because no source that fits its cutout gets there:
#   tile32 start 1:  d0 = n - 1 - t - 16 >= 32 needs t <= n - 49 < -16 for n <= 32, beyond -(n-1)/2
#   tile64 / wave8 start 1:  d0 = n - 1 - t - 32 >= 64 needs t <= n - 97 <= -33 for n <= 64, beyond -(n-1)/2
#   (fold start -1: on an axis of n >= 65, d0 < 0 needs t > n - 33 >= 32, and (n-1)/2 - 2.2 sigma <= 31 for n <= 85,
#    sigma = 5; the SHORT axis of a ragged fold-path cutout gets there -- n = 20, t > -13 -- so 85x20 and 20x85 are
#    in the list and start -1 is required of the fold path on both axes)
#   p192, general start 1:  the window is the whole period: d0 = l_c - P/2 < P/2 always; "a window end at or beyond
#       the period" is every start >= 0 there
#   general, y axis of 30x260:  P = 448, d0 = 29 - t - 224 < 0 for every t; the square shapes reach start 0 on y
REQUIRED = {
    'tile32': {'start': {-1, 0}, 'flip': {0, 1}, 'coarse_wrap': {0, 1}},
    'tile64': {'start': {-1, 0}, 'flip': {0, 1}, 'coarse_wrap': {0, 1}},
    'wave8': {'start': {-1, 0}, 'flip': {0, 1}, 'coarse_wrap': {0, 1}},
    'fold': {'start': {-1, 0, 1}, 'flip': {0, 1}, 'coarse_wrap': {0, 1}},
    'p192': {'start': {-1, 0}},
    'general': {'start': {-1, 0}},
}


def check_coverage(family):
    """the case list reaches every window class the family has, on both axes; returns the table row"""
    rows = []
    for axis in (0, 1):
        got, can = reached_classes(family, axis)
        need = dict(REQUIRED[family])
        if family == 'p192' and axis == 1:
            need['wrap_copy_columns'] = {0, 1, 2}
        for k, v in need.items():
            assert got.get(k, set()) >= v, (family, 'yx'[axis], k, got.get(k), v)
        for k, v in can.items():         # and nothing a fitting source can reach is missing
            assert got[k] >= v, (family, 'yx'[axis], k, got[k], v)
        rows.append((family, 'yx'[axis], {k: sorted(v) for k, v in got.items()}))
    if family in ('p192', 'general'):
        # the sign of the window start l_c - P/2 changes at a different distance from the centre for every size;
        # each square shape has it inside what its spot can reach, and the list is on both sides of it
        for ny, nx in FAMILIES[family]['shapes']:
            for axis in (0, 1):
                can = reachable_classes(family, ny, nx, axis)['start']
                n = (ny, nx)[axis]
                got = {window_class(family, ny, nx, axis, (n - 1) // 2 + int(np.floor(pr[1 - axis] + 0.5)))['start']
                       for up in FAMILIES[family]['ups'] for pr in shifts(ny, nx, up)}
                assert got == can, (family, ny, nx, axis, got, can)
                if ny == nx:
                    assert can == {-1, 0}, (family, ny, nx, can)
    return rows


# ---------------------------------------------------------------------------------------------------------------
# tolerances: the project's own (tests/test_gpu_parity.py, tests/test_refine_roll_cpu.py), unchanged
# ---------------------------------------------------------------------------------------------------------------
def tolerance(family, ny, nx, up, refine):
    if up == 1:
        return 1e-5
    if family == 'general':
        return 3e-4
    if up == 2:
        return 2e-5
    f32 = max(ny, nx) <= 85 and refine != 'float64'        # the 32 tile and the 64 tile's default refine in float32
    if f32:
        return 3e-4 if up >= 27 else 2e-4
    return 1e-4


MEASURED = {}        # (family or reference-mode kernel, refine form or input type, upsample) -> worst |kernel - oracle|
                     # seen by the checks in this process


def check_pair_cell(backend, family, shape, up, cc):
    """every refine form of the family against the oracle: status 0 and equal on both sides for every pair, the
    shifts within the family's tolerance.  `backend.select` may take fewer pairs of a cell (CPU threads, where a
    pair costs a tenth of a second and more); at upsample 1 the refine stage does not run, so one form is run."""
    ny, nx = shape
    sel = backend.select(len(shifts(ny, nx, up)), up, cc)
    ref, img = pairs(ny, nx, up)
    ref, img = ref[list(sel)], img[list(sel)]
    exp, est = oracle_pairs(ny, nx, up, cc, sel)
    assert np.all(est == 0), (family, shape, up, cc, est)
    for refine in FAMILIES[family]['refines'][:1 if up == 1 else None]:
        got, st = backend.pair(ref, img, up, cc, family, refine)
        err = float(np.max(np.abs(got - exp)))
        print('%s %dx%d upsample %d %s refine %s: %d pairs, worst |kernel - oracle| %.2e px'
              % (family, ny, nx, up, cc, refine, len(ref), err))
        key = (family, refine, up)
        MEASURED[key] = max(MEASURED.get(key, 0.0), err)
        assert np.array_equal(st, est), (family, shape, up, cc, refine, st)
        tol = tolerance(family, ny, nx, up, refine)
        assert err < tol, (family, shape, up, cc, refine, err, tol, np.abs(got - exp).max(axis=1))


def pair_cells(family):
    fam = FAMILIES[family]
    return [(s, up, cc) for s in fam['shapes'] for up in fam['ups'] for cc in CC_TYPES]


def measured_table(backend, families):
    """the table of profiles/r08/peak_window.txt for this backend, from what the checks of this process measured
    (a row the process did not run is left out); every figure is inside its tolerance"""
    lines = ['%-10s %-8s %8s %10s %12s' % ('family', 'refine', 'upsample', 'tolerance', backend.name)]
    for family in families:
        fam = FAMILIES[family]
        for refine in fam['refines']:
            for up in fam['ups']:
                if up == 1 and refine != fam['refines'][0]:
                    continue
                tol = max(tolerance(family, ny, nx, up, refine) for ny, nx in fam['shapes'])
                if (family, refine, up) not in MEASURED:
                    continue
                assert MEASURED[(family, refine, up)] < tol
                lines.append('%-10s %-8s %8d %10.0e %12.2e' % (family, refine, up, tol, MEASURED[(family, refine, up)]))
    for key in sorted(k for k in MEASURED if k[0] in DISP5_SHAPES):
        assert MEASURED[key] < DISP5_TOL
        lines.append('%-10s %-8s %8d %10.0e %12.2e' % (key + (DISP5_TOL, MEASURED[key])))
    return '\n'.join(lines)


# ---------------------------------------------------------------------------------------------------------------
# reference mode (find_displacement_batch / find_displacement_var): one size per kernel
# ---------------------------------------------------------------------------------------------------------------
DISP5_SHAPES = {'disp5_32': (20, 20), 'disp5p': (40, 40), 'disp5_fold': (80, 80), 'disp5_128': (100, 100),
                'disp5_big': (150, 150)}
DISP5_TOL = 3e-5                                                   # tests/test_gpu_parity.py goldens


@functools.lru_cache(maxsize=None)
def dithers(ny, nx, dtype):
    """the interlaced image is the upsample-2 grid: the same swept shifts, ties of that grid left out"""
    sg = sigma_for(ny, nx)
    sets = [datagen.dither_set(ny, nx, tx, ty, sg, amp=1.3, dtype=np.dtype(dtype)) for tx, ty in shifts(ny, nx, 2)]
    ref = np.stack([s[0] for s in sets])
    im4 = np.stack([np.stack(s[1:]) for s in sets])
    ref.setflags(write=False)
    im4.setflags(write=False)
    return ref, im4


@functools.lru_cache(maxsize=None)
def oracle_dithers(ny, nx, dtype, cc):
    ref, im4 = dithers(ny, nx, dtype)
    return orc.find_displacement_batch(ref, im4, cc)


def check_disp5(backend, kernel, cc, dtype):
    ny, nx = DISP5_SHAPES[kernel]
    ref, im4 = dithers(ny, nx, dtype)
    exp, est = oracle_dithers(ny, nx, dtype, cc)
    assert np.all(est == 0), (kernel, cc, est)
    got, st = backend.disp5(ref, im4, cc)
    err = float(np.max(np.abs(got - exp)))
    print('%s %dx%d %s %s: %d sources, worst |kernel - oracle| %.2e px' % (kernel, ny, nx, cc, dtype, len(ref), err))
    MEASURED[(kernel, dtype, 2)] = max(MEASURED.get((kernel, dtype, 2), 0.0), err)
    assert np.array_equal(st, est), (kernel, cc, dtype, st)
    assert err < DISP5_TOL, (kernel, cc, dtype, err)
    if backend.var_max_side is None or max(ny, nx) <= backend.var_max_side:
        # find_displacement_var (float32 and float64 entries): the same sources, each cut to a shape of its own inside the family (one row
        # and one column less for every second source; the spot keeps its 2.2 sigma, less one pixel)
        refs = [ref[k][:ny - k % 2, :nx - k % 2] for k in range(len(ref))]
        im4s = [im4[k][:, :ny - k % 2, :nx - k % 2] for k in range(len(ref))]
        e = [orc.find_displacement(r, *m, cc_type=cc, _status=s) + (s[-1],)
             for r, m, s in ((r, m, []) for r, m in zip(refs, im4s))]
        ev, es = np.array([x[:2] for x in e]), np.array([x[2] for x in e], np.int32)
        gv, gs = backend.disp5_var(refs, im4s, cc, max(ny, nx))
        assert np.all(es == 0) and np.array_equal(gs, es), (kernel, cc, gs, es)
        assert np.max(np.abs(gv - ev)) < DISP5_TOL, (kernel, cc, np.max(np.abs(gv - ev)))


# ---------------------------------------------------------------------------------------------------------------
# correlation peaks on the borders of the 'same' window, for one size per family (test_pair_mode_edge_cases has
# 64 px): delta functions at lag ref - img; q = 0 <-> lag +((n-1)//2) (centroid.py:171 edge rule), q = n-1 <->
# lag -(n//2) (off-centre fit box, centroid.py:175-184)
# ---------------------------------------------------------------------------------------------------------------
BORDER_SIZES = (20, 80, 100, 150)
INTERIOR_LAGS = ((0, 0), (-4, 7))
ST_EDGE = 1


def border_pairs(n):
    h, g = (n - 1) // 2, n // 2

    def deltas(ly, lx):
        ref, img = np.zeros((n, n), np.float32), np.zeros((n, n), np.float32)
        iy, ix = max(0, -ly) + (n - 1 - abs(ly)) // 2, max(0, -lx) + (n - 1 - abs(lx)) // 3
        img[iy, ix] = 1
        ref[iy + ly, ix + lx] = 1
        return ref, img
    lags = [(h, h), (-g, -g), (-(g - 1), h), (h, -(g - 1)), (0, h), (h, 0), (-g, 5), (3, -g), (0, 0), (-4, 7)]
    prs = [(np.zeros((n, n), np.float32),) * 2, (np.ones((n, n), np.float32),) * 2] + [deltas(*l) for l in lags]
    edge = [0] + [2 + k for k, (ly, lx) in enumerate(lags) if ly == h or lx == h]      # first row / first column
    return np.stack([p[0] for p in prs]), np.stack([p[1] for p in prs]), [(None, None)] * 2 + lags, edge


def check_borders(backend, n):
    ref, img, lags, edge = border_pairs(n)
    family = family_of(n, n)
    for up in (1, 2, 10):
        exp, est = orc.xcorr_refine_batch(ref, img, up, full_grid=True)
        for refine in FAMILIES[family]['refines']:
            got, st = backend.pair(ref, img, up, 'CC', family, refine)
            assert np.array_equal(st, est), (n, up, refine, st, est)
            assert np.max(np.abs(got - exp)) < 1e-3, (n, up, refine, got, exp)
            assert np.all(st[edge] == ST_EDGE), (n, up, st, edge)
            for k, (ly, lx) in enumerate(lags):
                if (ly, lx) in INTERIOR_LAGS:               # an interior lag comes back as the shift img - ref
                    assert st[k] == 0 and abs(got[k, 0] + lx) < 1e-3 and abs(got[k, 1] + ly) < 1e-3, (n, up, k, got[k])


# ---------------------------------------------------------------------------------------------------------------
# batch behaviour: a permuted batch gives the permuted result bit for bit; in a batch larger than the grid every
# item gives what it gives alone (the grid-stride loop carries nothing from the previous item: peak, window
# centre, tables)
# ---------------------------------------------------------------------------------------------------------------
BATCH_CELLS = {'tile32': ((20, 20), 10), 'tile64': ((40, 40), 10), 'wave8': ((40, 40), 10), 'fold': ((80, 80), 10),
               'p192': ((100, 100), 10), 'general': ((129, 129), 10)}


def check_batch(backend, family):
    (ny, nx), up = BATCH_CELLS[family]
    ref, img = pairs(ny, nx, up)
    sel = list(backend.batch_select(len(ref)))
    ref, img = ref[sel], img[sel]
    refine = FAMILIES[family]['refines'][0]
    base, bst = backend.pair(ref, img, up, 'CC', family, refine)
    perm = np.random.default_rng(7).permutation(len(ref))
    got, st = backend.pair(ref[perm], img[perm], up, 'CC', family, refine)
    assert np.array_equal(got, base[perm]) and np.array_equal(st, bst[perm]), family
    alone = np.concatenate([backend.pair(ref[k:k + 1], img[k:k + 1], up, 'CC', family, refine)[0] for k in range(len(ref))])
    assert np.array_equal(alone, base), family
    # neighbours in the stride loop are far apart in the sweep: opposite ends of the window follow each other
    idx = backend.overflow_index(family, len(ref))
    got, st = backend.pair_gathered(ref, img, idx, up, 'CC', family, refine)
    assert np.array_equal(got, base[idx]) and np.array_equal(st, bst[idx]), family


# ---------------------------------------------------------------------------------------------------------------
# backends
# ---------------------------------------------------------------------------------------------------------------
class EmuBackend:
    """the kernel source on CPU threads (tests/emu.py), each family forced with `tile=`"""
    name = 'CPU threads'
    GRID = 3
    var_max_side = 128          # the harness has the packed-catalog entry only, which stops at 128 px

    def select(self, count, up, cc):
        """pairs of a cell run on CPU threads: all of them for CC at upsample 10 (the sweep, then the sub-pixel
        positions); else every second pair of the nine-shift sweep (both ends and the middle), for ZNCC the ends and
        the middle.  The device backend runs every pair of every cell."""
        if cc == 'CC' and up == 10:
            return tuple(range(count))
        return (0, 2, 4, 6, 8) if cc == 'CC' else (0, 4, 8)

    def batch_select(self, count):
        return tuple(range(0, count, 2))

    def pair(self, ref, img, up, cc, family, refine):
        import emu
        code = {'CC': 0, 'NCC': 1, 'ZNCC': 2}[cc]
        try:
            emu.set_refine64({'default': -1, 'float32': 0, 'float64': 1}[refine])
            return emu.pair(ref, img, up, code, FAMILIES[family]['tile'])
        finally:
            emu.set_refine64(-1)

    def overflow_index(self, family, count):
        """every item three times over a grid of 3 workgroups (the 32 tile: 4 pairs each)"""
        rng = np.random.default_rng(11)
        return np.concatenate([rng.permutation(count) for _ in range(3)])

    def pair_gathered(self, ref, img, idx, up, cc, family, refine):
        import emu
        try:
            emu.set_grid(self.GRID)
            return self.pair(ref[idx], img[idx], up, cc, family, refine)
        finally:
            emu.set_grid(0)

    def disp5(self, ref, im4, cc):
        import emu
        out, st, _ = emu.disp5(ref, im4, {'CC': 0, 'NCC': 1, 'ZNCC': 2}[cc])
        return out, st

    def disp5_var(self, refs, im4s, cc, family_side):
        import emu
        out, st, _ = emu.disp5_var(refs, im4s, family_side, {'CC': 0, 'NCC': 1, 'ZNCC': 2}[cc])
        return out, st


class GpuBackend:
    """subpixal_amd on the device; the product's dispatch picks the family from the shape (the eight-wave kernel:
    a process started with SPX_PAIR64_WAVES=8)"""
    name = 'MI355X'
    var_max_side = None         # cc.find_displacement_var takes every size (above 128 px: one launch per shape)

    def select(self, count, up, cc):
        return tuple(range(count))

    def batch_select(self, count):
        return tuple(range(count))

    def pair(self, ref, img, up, cc, family, refine):
        import subpixal_amd as spx
        assert family_of(*ref.shape[1:]) == ('tile64' if family == 'wave8' else family)
        assert (os.environ.get('SPX_PAIR64_WAVES') == '8') == (family == 'wave8'), family
        return spx.xcorr_refine_batch(ref, img, upsample=up, cc_type=cc, return_status=True, refine=refine)

    def overflow_index(self, family, count):
        """more items than the largest grid the host launches for the family (spx_capi.hip: 32 workgroups per
        CU for the 32 and 64 tiles, four pairs to a workgroup on the 32 tile; 2 per CU above 85 px)"""
        import torch
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        grid = {'tile32': 4 * 32 * cus, 'tile64': 32 * cus, 'wave8': 32 * cus, 'fold': 32 * cus,
                'p192': 2 * cus, 'general': 2 * cus}[family]
        return np.random.default_rng(11).integers(0, count, grid + grid // 8 + 5)

    def pair_gathered(self, ref, img, idx, up, cc, family, refine):
        """the batch is put together on the device from the cell's few pairs"""
        import torch
        import subpixal_amd as spx
        from subpixal_amd import device
        dev = 'cuda:%d' % device.init()
        i = torch.as_tensor(idx).to(dev)
        r = torch.as_tensor(np.ascontiguousarray(ref)).to(dev)[i].contiguous()
        m = torch.as_tensor(np.ascontiguousarray(img)).to(dev)[i].contiguous()
        got, st = spx.xcorr_refine_batch(r, m, upsample=up, cc_type=cc, return_status=True, refine=refine)
        return got.cpu().numpy(), st.cpu().numpy()

    def disp5(self, ref, im4, cc):
        import subpixal_amd as spx
        return spx.find_displacement_batch(ref, im4, cc_type=cc, return_status=True)

    def disp5_var(self, refs, im4s, cc, family_side):
        import subpixal_amd as spx
        return spx.find_displacement_var(refs, im4s, cc_type=cc, return_status=True)


def run_family(backend, family):
    """every check of one family in this process (the eight-wave kernel's child process)"""
    for shape, up, cc in pair_cells(family):
        check_pair_cell(backend, family, shape, up, cc)
    check_batch(backend, family)
    print(measured_table(backend, [family]))


def run_family_in_child(family, env, timeout):
    """a fresh process (never exec: the parent may hold the device) that runs `run_family` on the device"""
    code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n'
            'import peak_cases as pc\npc.run_family(pc.GpuBackend(), %r)\nprint("peak window child OK")\n'
            % (ROOT, os.path.join(ROOT, 'tests'), family))
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, **env), capture_output=True, text=True,
                         timeout=timeout)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-4000:]
    assert 'peak window child OK' in out.stdout
    return out.stdout
