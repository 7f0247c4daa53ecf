"""The float64 catalog path without a GPU: the four C entries behind it (spx_gather_cutouts_f64,
spx_gather_cutouts_var_f64, spx_blot4_var_to_f64, spx_find_displacement5_catalog_f64) are exported, declared and
check their arguments before any HIP call; the float64 gathers and blots run on CPU threads
(tests/cpu_emu/emu_catalog_f64.cpp) against a numpy statement of the reference's Cutout rules."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'subpixal_amd', 'csrc')
NEW = ('spx_gather_cutouts_f64', 'spx_gather_cutouts_var_f64', 'spx_blot4_var_to_f64',
       'spx_find_displacement5_catalog_f64')
E_ARG, E_WORKSPACE = -1, -4


def _declared():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'subpixal_hip.h')).read(), flags=re.S)
    return set(re.findall(r'\b(spx_[a-z0-9_]+)\s*\(', text))


def test_new_entries_exported_and_declared():
    from subpixal_amd import _ffi
    lib = _ffi.load()
    declared = _declared()
    for name in NEW:
        assert name in declared and name in _ffi.EXPORTED_SYMBOLS, name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.spx_abi_version() == _ffi.ABI_VERSION == 4


def test_argument_errors_before_any_hip_call():
    from subpixal_amd import _ffi
    lib = _ffi.load()
    buf64, buf32 = np.zeros(256, np.float64), np.zeros(256, np.float32)
    ib, lb = np.zeros(256, np.int32), np.zeros(256, np.int64)
    i, l = ib.ctypes.data, lb.ctypes.data
    for f64 in (False, True):
        b = (buf64 if f64 else buf32).ctypes.data
        g = lib.spx_gather_cutouts_f64 if f64 else lib.spx_gather_cutouts_f32
        gv = lib.spx_gather_cutouts_var_f64 if f64 else lib.spx_gather_cutouts_var_f32
        bl = lib.spx_blot4_var_to_f64 if f64 else lib.spx_blot4_var_f32
        cat = lib.spx_find_displacement5_catalog_f64 if f64 else lib.spx_find_displacement5_catalog_f32
        # null pointers / negative batch
        assert g(None, None, 8, 8, i, 1, 4, 4, 0.0, b, None, None, None) == E_ARG
        assert g(b, None, 8, 8, i, -1, 4, 4, 0.0, b, None, None, None) == E_ARG
        assert gv(b, None, 8, 8, None, 1, l, 0.0, b, None, None, None) == E_ARG
        assert gv(b, None, 8, 8, i, -1, l, 0.0, b, None, None, None) == E_ARG
        assert bl(b, l, i, 1, None, 0, None, l, i, b, None) == E_ARG
        assert bl(b, l, i, -1, b, 0, None, l, i, b, None) == E_ARG
        assert cat(b, None, l, i, 1, 1, 1, b, i, b, None, 0, None) == E_ARG
        assert cat(b, b, l, i, -1, 1, 1, b, i, b, None, 0, None) == E_ARG
        # seg without ids
        assert g(b, None, 8, 8, i, 1, 4, 4, 0.0, b, i, None, None) == E_ARG
        assert gv(b, None, 8, 8, i, 1, l, 0.0, b, i, None, None) == E_ARG
        # family_mask outside bits 0..3, blot degree 6
        assert cat(None, None, None, None, 0, 16, 1, None, None, None, None, 0, None) == E_ARG
        assert bl(None, None, None, 0, None, 6, None, None, None, None, None) == E_ARG
        # an empty batch is a no-op
        assert g(None, None, 8, 8, None, 0, 4, 4, 0.0, None, None, None, None) == 0
        assert gv(None, None, 8, 8, None, 0, None, 0.0, None, None, None, None) == 0
        assert bl(None, None, None, 0, None, 0, None, None, None, None, None) == 0
        assert cat(None, None, None, None, 0, 15, 1, None, None, None, None, 0, None) == 0
        # family bit 3 (86..128 px) without its workspace
        assert lib.spx_workspace_bytes_xcorr(1, 128, 128) > 0
        assert cat(b, b, l, i, 1, 8, 1, b, i, b, None, 0, None) == E_WORKSPACE


# ---------------------------------------------------------------------------------------------------------------
# the kernels on CPU threads
# ---------------------------------------------------------------------------------------------------------------
_LIB = {}


@pytest.fixture(scope='module')
def emu64(tmp_path_factory):
    """tests/cpu_emu/emu_catalog_f64.cpp built with the Makefile's emu compiler and flags"""
    if 'lib' not in _LIB:
        out = subprocess.check_output(['make', '-s', '-C', CSRC, '--eval',
                                       'spx-emu-flags: ; @echo $(HOSTCXX) $(EMUFLAGS)', 'spx-emu-flags'],
                                      universal_newlines=True).split()
        so = str(tmp_path_factory.mktemp('emu64') / 'libspx_emu_catalog_f64.so')
        subprocess.check_call(out + ['-shared', '-o', so, os.path.join(ROOT, 'tests', 'cpu_emu',
                                                                      'emu_catalog_f64.cpp')])
        _LIB['lib'] = ctypes.CDLL(so)
    return _LIB['lib']


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _cutout_rules(frame, box, fill, fmask=None, seg=None, sid=None):
    """numpy statement of a cutout's pixels: the reference's Cutout(mode='fill') (cutout.py:737-755) with the
    bad-pixel mask, the foreign-segment mask (cutout.py:190) and non-finite pixels set to `fill`"""
    x0, y0, w, h = (int(v) for v in box)
    fny, fnx = frame.shape
    out = np.full((h, w), fill, frame.dtype)
    ys, xs = np.mgrid[y0:y0 + h, x0:x0 + w]
    inside = (xs >= 0) & (xs < fnx) & (ys >= 0) & (ys < fny)
    yy, xx = ys[inside], xs[inside]
    v = frame[yy, xx]
    bad = ~np.isfinite(v)
    if fmask is not None:
        bad |= fmask[yy, xx]
    if seg is not None:
        bad |= seg[yy, xx] != sid
    out[inside] = np.where(bad, fill, v)
    return out


def _scene():
    rng = np.random.default_rng(31)
    fny, fnx = 70, 90
    k = rng.integers(1, 2 ** 20, (fny, fnx)).astype(np.float64)
    frame = 1.0 + k * 2.0 ** -40                      # in-frame values float32 cannot represent
    frame[::3] = rng.standard_normal((len(frame[::3]), fnx)) * 1e4 + 1e-7
    frame[10, 12], frame[11, 13], frame[12, 14] = np.nan, np.inf, -np.inf
    fmask = rng.random((fny, fnx)) < 0.03
    seg = np.where(rng.random((fny, fnx)) < 0.6, 4, 9).astype(np.int32)
    boxes = np.array([[5, 6, 20, 15], [-6, -3, 17, 12], [80, 60, 18, 14], [8, 8, 9, 7], [30, -10, 4, 90],
                      [-20, 20, 11, 11]], np.int32)   # overhanging on every side; one fully outside in x
    ids = np.array([4, 9, 4, 4, 9, 4], np.int32)
    return frame, fmask, seg, boxes, ids


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize('fill', [0.0, np.nan, -3.5])
def test_f64_gathers_follow_the_cutout_rules_bit_for_bit(emu64, fill):
    frame, fmask, seg, boxes, ids = _scene()
    fny, fnx = frame.shape
    n = len(boxes)
    i32 = boxes.ctypes.data_as(ctypes.c_void_p)
    m8 = np.ascontiguousarray(fmask, np.uint8)
    sizes = boxes[:, 2].astype(np.int64) * boxes[:, 3]
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    tny, tnx = int(boxes[:, 3].max()), int(boxes[:, 2].max())
    for masked in (False, True):
        fm = m8 if masked else None
        sg, si = (seg, ids) if masked else (None, None)
        # variable-shape gather
        out = np.full(int(sizes.sum()), -7.0)
        assert emu64.emu64_gather_var(_ptr(frame), _ptr(fm), fny, fnx, i32, ctypes.c_int64(n), _ptr(offs),
                                      ctypes.c_double(fill), _ptr(out), _ptr(sg), _ptr(si)) == 0
        # fixed-shape gather: padding outside the window is 0
        tiles = np.full((n, tny, tnx), -7.0)
        assert emu64.emu64_gather(_ptr(frame), _ptr(fm), fny, fnx, i32, ctypes.c_int64(n), tny, tnx,
                                  ctypes.c_double(fill), _ptr(tiles), _ptr(sg), _ptr(si)) == 0
        for k, box in enumerate(boxes):
            want = _cutout_rules(frame, box, fill, fmask if masked else None, sg, None if si is None else si[k])
            h, w = want.shape
            assert _same_bits(out[offs[k]:offs[k] + h * w].reshape(h, w), want), (k, masked)
            pad = np.zeros((tny, tnx))
            pad[:h, :w] = want
            assert _same_bits(tiles[k], pad), (k, masked)
    # the float64 values survive: float32 would have rounded them
    v = out[offs[0]:offs[0] + sizes[0]]
    v = v[np.isfinite(v)]
    assert np.count_nonzero(v != v.astype(np.float32)) > 0.5 * v.size


def test_f64_blots_are_the_f32_blots_widened(emu64):
    rng = np.random.default_rng(32)
    src_shapes = np.array([[20, 25], [14, 9], [5, 30], [33, 40]], np.int32)   # the third: too small to resample
    dst_shapes = np.array([[12, 15], [10, 7], [6, 6], [25, 31]], np.int32)
    n = len(src_shapes)

    def layout(shapes):
        sizes = shapes[:, 0].astype(np.int64) * shapes[:, 1]
        return np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64), int(sizes.sum())
    soffs, stot = layout(src_shapes)
    doffs, dtot = layout(dst_shapes)
    src = (rng.standard_normal(stot) * 1e3 + 5e3).astype(np.float32)
    aff = np.stack([np.array([1.01, 0.02, 2.3 + 0.4 * k, -0.01, 0.98, 1.7 - 0.2 * k]) for k in range(n)])
    coef = np.zeros((n, 2, 21))
    coef[:, 0, 0], coef[:, 1, 0] = 6.0, 5.5
    coef[:, 0, 1], coef[:, 1, 2] = 0.97, 1.02
    coef[:, 0, 4], coef[:, 1, 3] = 1e-3, -2e-3
    gain = np.array([1.0, 0.37, 2.0, 1.5], np.float32)
    for maps, degree in ((aff, 0), (coef, 3)):
        for g in (None, gain):
            o32 = np.full(4 * dtot, -7.0, np.float32)
            o64 = np.full(4 * dtot, -7.0, np.float64)
            args = (_ptr(src), _ptr(soffs), _ptr(src_shapes), ctypes.c_int64(n), _ptr(maps), degree, _ptr(g),
                    _ptr(doffs), _ptr(dst_shapes))
            assert emu64.emu64_blot4_var_f32(*args, _ptr(o32)) == 0
            assert emu64.emu64_blot4_var_to_f64(*args, _ptr(o64)) == 0
            assert not np.any(o32 == -7.0) and o32.any()
            assert _same_bits(o64, o32.astype(np.float64)), (degree, g is None)
            k = 2                                                             # no signal from a 5-px source
            assert not o64[4 * doffs[k]:4 * doffs[k] + 4 * 36].any()
