"""A pair's result does not depend on whether its predecessor staged it (spx_kernels.h pair_body: on full
64x64 float32 tiles, float32 refine with one window block, plain CC, a pair writes its SUCCESSOR into the staging
region during its own refine stage, and the successor then skips its staging).  Run on CPU threads by the
logic-check harness (tests/cpu_emu): a batch walked by 2 workgroups -- 3-4 pairs each, every pair but the first of
a walk staged by the one before it -- against the same pairs sent one per call, where no pair has a predecessor.
The comparison is for equality: both ways are the same operations on the same values.

With 2 workgroups the walk is linear (first_item: launches that are no multiple of 64 workgroups): workgroup 0 takes
pairs 0, 2, 4, 6 and workgroup 1 takes 1, 3, 5."""
import functools

import numpy as np
import pytest

import datagen
import emu
import peak_cases
from oracle import subpixal_oracle as orc

COUNT, GRID = 7, 2
ST_NONFINITE = 6


def _walked(ref, img, up, cc=0):
    try:
        emu.set_grid(GRID)
        return emu.pair(ref, img, up, cc)
    finally:
        emu.set_grid(0)


def _alone(ref, img, up, cc=0):
    res = [emu.pair(ref[k:k + 1], img[k:k + 1], up, cc) for k in range(len(ref))]
    return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])


@functools.lru_cache(maxsize=None)
def _batch(n=64):
    ref, img, truth = datagen.pair_batch(41, COUNT, n)
    for a in (ref, img, truth):
        a.setflags(write=False)
    return ref, img, truth


@functools.lru_cache(maxsize=None)
def _alone_base(up):
    ref, img, _ = _batch()
    return _alone(ref, img, up)


def _same(a, b):
    """bit for bit, NaN included"""
    return np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1])


def test_walk_positions():
    assert emu.first_item(0, GRID) == 0 and emu.first_item(1, GRID) == 1


@pytest.mark.parametrize('up', [10, 11, 12])      # 10, 11: one window block (stage-ahead); 12: two blocks (each pair stages itself)
def test_walked_batch_equals_pairs_alone(up):
    ref, img, truth = _batch()
    got = _walked(ref, img, up)
    assert _same(got, _alone_base(up)), (up, got, _alone_base(up))
    assert np.all(got[1] == 0)
    assert np.max(np.abs(got[0] - truth)) < 1e-3


@pytest.mark.parametrize('where', [0, 2, 6])      # first, a middle and the last pair of workgroup 0's walk
def test_non_finite_pair_and_its_neighbours(where):
    """the non-finite pair skips its refine stage, so it stages nothing ahead and its successor stages itself;
    its predecessor staged it as any other pair"""
    ref, img, _ = _batch()
    ref, img = ref.copy(), img.copy()
    img[where, 17, 23] = np.nan
    got = _walked(ref, img, 10)
    exp = tuple(a.copy() for a in _alone_base(10))
    one = emu.pair(ref[where:where + 1], img[where:where + 1], 10)
    exp[0][where], exp[1][where] = one[0][0], one[1][0]
    assert one[1][0] == ST_NONFINITE
    assert _same(got, exp), (where, got, exp)
    # and with the NaN in the reference of the other workgroup's walk (pairs 1, 3, 5)
    if where == 2:
        ref, img, _ = _batch()
        ref, img = ref.copy(), img.copy()
        ref[3, 40, 5] = np.nan
        got = _walked(ref, img, 10)
        exp = tuple(a.copy() for a in _alone_base(10))
        exp[0][3], exp[1][3] = emu.pair(ref[3:4], img[3:4], 10)[0][0], ST_NONFINITE
        assert _same(got, exp), (got, exp)


def _recentres(ref, img, up):
    """mirror of pair_body's window decision at its first pass (float64): the 16 x 16 window of the fine grid
    centred on the coarse arg-max, its arg-max inside the virtual image, and whether the 5 x 5 fit box around that
    (clamped into the image) leaves the window -- then the kernel moves the window and builds it again"""
    ny, nx = ref.shape
    coarse = orc.upsampled_cc(ref, img, 1)
    qy, qx = np.unravel_index(np.argmax(coarse), coarse.shape)
    fine = orc.upsampled_cc(ref, img, up)
    fy0, fx0 = up * qy - 8, up * qx - 8
    ys = np.arange(max(fy0, 0), min(fy0 + 16, up * ny))
    xs = np.arange(max(fx0, 0), min(fx0 + 16, up * nx))
    win = fine[np.ix_(ys, xs)]
    a, b = np.unravel_index(np.argmax(win), win.shape)
    jmax, imax = int(ys[a]), int(xs[b])
    x1 = min(max(imax - 2, 0), up * nx - 5)
    y1 = min(max(jmax - 2, 0), up * ny - 5)
    okx = (x1 >= fx0 and x1 + 4 < fx0 + 16) or imax == 0
    oky = (y1 >= fy0 and y1 + 4 < fy0 + 16) or jmax == 0
    return not (okx and oky)


@functools.lru_cache(maxsize=None)
def _recentring_case():
    """(upsample, index) of the first pair of peak_cases' 64-tile list (64 x 64 cutouts) whose peak forces a
    re-centred window at an upsample of one window block.  (At upsample 10 a peak half a pixel from the coarse
    arg-max still has its fit box inside the window, 5 + 2 < 8 fine samples; at upsample 11 the list's half-pixel
    shifts put it at 6 + 2.)"""
    for up in (10, 11):
        ref, img = peak_cases.pairs(64, 64, 10)
        for k in range(len(ref)):
            if _recentres(ref[k].astype(np.float64), img[k].astype(np.float64), up):
                return up, k
    return None


def test_recentred_window_keeps_the_staged_pair():
    """a re-centred window rebuilds the fine window only: the successor staged during the first pass stays"""
    case = _recentring_case()
    assert case is not None, "peak_cases' 64 x 64 list has no pair that re-centres its window"
    up, k = case
    pref, pimg = peak_cases.pairs(64, 64, 10)
    for where in (0, 2, 6):
        ref, img, _ = _batch()
        ref, img = ref.copy(), img.copy()
        ref[where], img[where] = pref[k], pimg[k]
        got = _walked(ref, img, up)
        exp = tuple(a.copy() for a in _alone_base(up))
        one = emu.pair(ref[where:where + 1], img[where:where + 1], up)
        exp[0][where], exp[1][where] = one[0][0], one[1][0]
        assert one[1][0] == 0
        assert _same(got, exp), (up, k, where, got, exp)


@pytest.mark.parametrize('cc', [1, 2])            # NCC, ZNCC: the successor's statistics come first, no stage-ahead
def test_normalised_correlation_takes_the_old_path(cc):
    ref, img, truth = _batch()
    got = _walked(ref, img, 10, cc)
    assert _same(got, _alone(ref, img, 10, cc))
    # (against the float64 definition, not the drawn shift: the normalisation itself moves the peak of a spot on a
    #  zero background; tolerance of tests/test_refine_roll_cpu.py for the float32 refine at upsample 10)
    exp, est = orc.xcorr_refine_batch(ref, img, 10, {1: 'NCC', 2: 'ZNCC'}[cc])
    assert np.array_equal(got[1], est) and np.all(est == 0)
    assert np.max(np.abs(got[0] - exp)) < 3e-4, np.max(np.abs(got[0] - exp))


def test_float64_batch():
    ref, img, truth = _batch()
    ref, img = ref.astype(np.float64), img.astype(np.float64)
    got = _walked(ref, img, 10)
    assert _same(got, _alone(ref, img, 10))
    assert np.all(got[1] == 0) and np.max(np.abs(got[0] - truth)) < 1e-3


def test_tile_that_is_not_full():
    ref, img, _ = _batch()
    ref, img = np.ascontiguousarray(ref[:, :63, :]), np.ascontiguousarray(img[:, :63, :])
    got = _walked(ref, img, 10)
    assert _same(got, _alone(ref, img, 10))
    assert np.all(got[1] == 0)
