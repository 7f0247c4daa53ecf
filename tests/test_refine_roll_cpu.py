"""The float32 refine of the 64 tile on a fixed plane order (spx_kernels.h fine_window_rolled): the
A fragments are read in storage order and the roll by the coarse peak sits in the kernel tables
(spx_tables.h make_ktab, rolled section).  Run on CPU threads by the logic-check harness
(tests/cpu_emu), against the oracle and against the float64 refine, which still reads the
planes rolled by the peak (spx_kernels.h fine_window).

A plane row r stands for the convolution index m = r (mod 64) in [l_c - 32, l_c + 32); the
table offset and the sign of the odd class change where that range crosses a multiple of 64.
The cutout sizes below put l_c = conv_index(n, q) on both sides of every such crossing:
33..40 px reach l_c < 32 (negative window start), the fold path (80, 85 px) l_c >= 96."""
import numpy as np
import pytest

import datagen
import emu
from oracle import subpixal_oracle as orc


def _conv_index(n, q):
    return (n - 1 - q) + (n - 1) // 2


def _pairs(n, shifts, sigma):
    """one pair per (tx, ty) of `shifts`; ty runs through the shifts backwards so that both
    axes see every value"""
    refs, imgs = [], []
    for tx, ty in zip(shifts, shifts[::-1]):
        r, i = datagen.pair_set(n, n, tx, ty, sigma, amp=1.3)
        refs.append(r)
        imgs.append(i)
    return np.stack(refs), np.stack(imgs)


def _shifts(n):
    lim = (n - 1) / 2.0 - 9.0             # keep the spot inside both cutouts
    base = np.linspace(-lim, lim, 9)
    # and sub-pixel positions around the centre: half pixels move the fine peak next to the
    # edge of the window that the coarse peak centres
    return np.concatenate([base + 0.37, [-2.5, -0.5, 0.5, 1.5, 2.49]])


# (cutout side, upsample): upsample 2 and 10 take the rolled form (one window block), 27 (two blocks) the
# peak-rolled reads it replaced there, checked the same way
CASES = [(n, up) for n in (33, 40, 64, 80, 85) for up in (2, 10, 27)]


def test_cases_reach_every_plane_wrap():
    """window start d0 = l_c - 32 below 0, inside [0, 64) and at or above 64, on both axes"""
    seen = set()
    for n, _ in CASES:
        for s in _shifts(n):
            for q in {int(round((n - 1) / 2.0 + s)), int(round((n - 1) / 2.0 - s))}:
                if 0 <= q < n:
                    seen.add((_conv_index(n, q) - 32) >> 6)
    assert seen >= {-1, 0, 1}, seen


@pytest.mark.parametrize('n,up', CASES)
def test_rolled_refine_vs_oracle_and_float64_refine(n, up):
    ref, img = _pairs(n, _shifts(n), 4.0 if n < 48 else 5.0)
    exp, est = orc.xcorr_refine_batch(ref, img, up)
    try:
        emu.set_refine64(0)
        got, st = emu.pair(ref, img, up)
        emu.set_refine64(1)
        got64, st64 = emu.pair(ref, img, up)
    finally:
        emu.set_refine64(-1)
    assert np.array_equal(st, est), (st, est)
    assert np.array_equal(st64, est), (st64, est)
    ok = st == 0
    assert ok.sum() >= len(st) - 2, st
    # the float32 refine's accuracy on this population: up to ~2.2e-4 px from
    # upsample 10 on; a wrong roll or sign shows as a whole fine pixel (1/up)
    tol = 5e-5 if up == 2 else 3e-4
    assert np.max(np.abs(got[ok] - exp[ok])) < tol, (n, up, np.max(np.abs(got[ok] - exp[ok])))
    assert np.max(np.abs(got[ok] - got64[ok])) < tol, (n, up, np.max(np.abs(got[ok] - got64[ok])))


def test_rolled_refine_is_deterministic_and_batch_order_free():
    n, up = 80, 10
    ref, img = _pairs(n, _shifts(n), 5.0)
    a, sa = emu.pair(ref, img, up)
    perm = np.random.default_rng(7).permutation(len(ref))
    b, sb = emu.pair(ref[perm], img[perm], up)
    assert np.array_equal(a[perm], b) and np.array_equal(sa[perm], sb)
