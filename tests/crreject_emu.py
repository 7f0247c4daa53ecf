"""The cosmic-ray kernels on CPU threads for the tests: builds tests/cpu_emu/emu_crreject.cpp on the fly with the
Makefile's emu compiler and flags (as drizzle_emu.py builds its harness) and runs a case of crreject_cases.py through
it.  The same library holds the drizzle's harness, for the single-frame runs.  Not a test module.
SPX_EMU_CRREJECT_LIB: a pre-built harness."""
import ctypes
import os
import subprocess

import numpy as np

import crreject_statement as cs
import drizzle_emu as de
import drizzle_statement as ds

ROOT = de.ROOT
_LIB = {}
_vp, _int, _dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double


def load(tmp_path_factory):
    if 'lib' not in _LIB:
        so = os.environ.get('SPX_EMU_CRREJECT_LIB')
        if not so:
            out = subprocess.check_output(['make', '-s', '-C', de.CSRC, '--eval',
                                           'spx-emu-flags: ; @echo $(HOSTCXX) $(EMUFLAGS)', 'spx-emu-flags'],
                                          universal_newlines=True).split()
            so = str(tmp_path_factory.mktemp('emuz') / 'libspx_emu_crreject.so')
            subprocess.check_call(out + ['-shared', '-o', so, os.path.join(ROOT, 'tests', 'cpu_emu', 'emu_crreject.cpp')])
        lib = ctypes.CDLL(so)
        for fn in (lib.emuz_drizzle_f32, lib.emuz_drizzle_f64):
            fn.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _int, _dbl, _int, _dbl, _int, _int, _vp, _vp, _vp, _int]
        for fn in (lib.emuz_crr_median_f32, lib.emuz_crr_median_f64):
            fn.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _int, _dbl, _int, _int, _int, _int, _int, _vp, _vp, _int]
        for fn in (lib.emuz_crr_cr_f32, lib.emuz_crr_cr_f64):
            fn.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _int, _dbl, _int, _int, _vp, _vp, _int, _int, _dbl, _vp, _dbl,
                           _dbl, _dbl, _dbl, _dbl, _dbl, _vp, _vp, _int]
        _LIB['lib'] = lib
    return _LIB['lib']


def params(c):
    p = dict(cs.DEFAULTS)
    p.update(c.get('cr', {}))
    return p


def actives(c):
    K = len(c['frames'])
    return [True] * K if c['active'] is None else [bool(a) for a in c['active']]


def singles(lib, c, dtype):
    """item 1 through the EXISTING drizzle harness: one run per frame with only that frame active; float32 values and
    the ctx bit as `valid`"""
    K = len(c['frames'])
    NY, NX = c['out_shape']
    vals, valid = np.zeros((K, NY, NX), np.float32), np.zeros((K, NY, NX), bool)
    for k, on in enumerate(actives(c)):
        if on:
            sci, wht, ctx = de.run(lib, dict(c, active=[int(q == k) for q in range(K)]), dtype)
            valid[k] = ds.ctx_bits(ctx, K)[k]
            vals[k] = np.where(valid[k], sci, 0).astype(np.float32)
    return vals, valid


def run_median(lib, c, dtype, grid=0):
    frames, weights, masks, shapes, maps, active, K = de.arrays(c, dtype)
    NY, NX = c['out_shape']
    p = params(c)
    med = np.full((NY, NX), -77.0, np.float32)
    nmed = np.full((NY, NX), 201, np.uint8)
    ft, wt, mt = de.pointer_table(frames, K), de.pointer_table(weights, K), de.pointer_table(masks, K)
    fn = lib.emuz_crr_median_f64 if np.dtype(dtype) == np.float64 else lib.emuz_crr_median_f32
    rc = fn(de._p(ft), de._p(wt), de._p(mt), de._p(shapes), de._p(maps), de._p(active), K, float(c['pixfrac']),
            ds.KERNELS[c['kernel']], p['nlow'], p['nhigh'], NY, NX, de._p(med), de._p(nmed), grid)
    assert rc == 0, rc
    return med, nmed


def rms_args(c, k, dtype):
    """(scalar, map or None) of frame k"""
    r = c['rms'][k]
    if np.isscalar(r):
        return float(r), None
    return 0.0, np.ascontiguousarray(r, dtype)


def run_cr(lib, c, dtype, k, med, nmed, grid=0):
    frames, weights, masks, shapes, maps, active, K = de.arrays(c, dtype)
    NY, NX = c['out_shape']
    p = params(c)
    ny, nx = frames[k].shape
    crmask = np.full((ny, nx), 201, np.uint8)
    clean = np.full((ny, nx), -77.0, dtype)
    ft, wt, mt = de.pointer_table(frames, K), de.pointer_table(weights, K), de.pointer_table(masks, K)
    rs, rm = rms_args(c, k, dtype)
    fn = lib.emuz_crr_cr_f64 if np.dtype(dtype) == np.float64 else lib.emuz_crr_cr_f32
    rc = fn(de._p(ft), de._p(wt), de._p(mt), de._p(shapes), de._p(maps), de._p(active), K, float(c['pixfrac']),
            ds.KERNELS[c['kernel']], k, de._p(med), de._p(nmed), NY, NX, rs, de._p(rm), float(p['sky']),
            float('nan') if p['gain'] is None else float(p['gain']), p['snr'][0], p['snr'][1], p['scale'][0],
            p['scale'][1], de._p(crmask), de._p(clean), grid)
    assert rc == 0, rc
    return crmask, clean


_ST = {}


def statement(name, c, vals, valid, dtype):
    """the statement of a named case and dtype, computed once and shared (read-only)"""
    key = (name, np.dtype(dtype).name)
    if key not in _ST:
        _ST[key] = cs.statement(c, vals, valid)
    return _ST[key]
