"""The kernels of spx_minmed_kernels.h on CPU threads for the tests: builds tests/cpu_emu/emu_minmed.cpp on the fly with
the Makefile's emu compiler and flags (as crreject_emu.py builds its harness) and runs a case of minmed_cases.py
through it.  The same library holds the drizzle's, the median's and the comparison's harness.  Not a test module.
SPX_EMU_MINMED_LIB: a pre-built harness."""
import ctypes
import os
import subprocess

import numpy as np

import crreject_emu as ce
import drizzle_emu as de
import drizzle_statement as ds
import minmed_statement as ms

ROOT = de.ROOT
_LIB = {}
_vp, _int, _dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double


def load(tmp_path_factory):
    if 'lib' not in _LIB:
        so = os.environ.get('SPX_EMU_MINMED_LIB')
        if not so:
            out = subprocess.check_output(['make', '-s', '-C', de.CSRC, '--eval',
                                           'spx-emu-flags: ; @echo $(HOSTCXX) $(EMUFLAGS)', 'spx-emu-flags'],
                                          universal_newlines=True).split()
            so = str(tmp_path_factory.mktemp('emuz') / 'libspx_emu_minmed.so')
            subprocess.check_call(out + ['-shared', '-o', so, os.path.join(ROOT, 'tests', 'cpu_emu', 'emu_minmed.cpp')])
        lib = ctypes.CDLL(so)
        for fn in (lib.emuz_drizzle_f32, lib.emuz_drizzle_f64):
            fn.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _int, _dbl, _int, _dbl, _int, _int, _vp, _vp, _vp, _int]
        for fn in (lib.emuz_crr_median_f32, lib.emuz_crr_median_f64):
            fn.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _int, _dbl, _int, _int, _int, _int, _int, _vp, _vp, _int]
        for fn in (lib.emuz_crr_cr_f32, lib.emuz_crr_cr_f64):
            fn.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _int, _dbl, _int, _int, _vp, _vp, _int, _int, _dbl, _vp, _dbl,
                           _dbl, _dbl, _dbl, _dbl, _dbl, _vp, _vp, _int]
        for fn in (lib.emuz_mm_minmed_f32, lib.emuz_mm_minmed_f64):
            fn.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _int, _dbl, _int, _int, _int, _vp, _dbl, _dbl, _int, _int, _int,
                           _vp, _vp, _vp, _vp, _vp, _vp, _int]
        for fn in (lib.emuz_mm_cr_grow_f32, lib.emuz_mm_cr_grow_f64):
            fn.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _int, _dbl, _int, _int, _vp, _vp, _int, _int, _dbl, _vp, _vp,
                           _int, _int, _int, _vp, _vp, _int]
        _LIB['lib'] = lib
    return _LIB['lib']


def mm_params(c):
    p = dict(ms.DEFAULTS)
    p.update(c.get('mm', {}))
    return p


def run_minmed(lib, c, dtype, grid=0):
    """dict(md, lo, bits, med, nmed, minmed) of the two launches"""
    frames, weights, masks, shapes, maps, active, K = de.arrays(c, dtype)
    NY, NX = c['out_shape']
    p, q = ce.params(c), mm_params(c)
    table = np.ascontiguousarray(ms.table_of(c))
    out = dict(md=np.full((NY, NX), -77.0, np.float32), lo=np.full((NY, NX), -77.0, np.float32),
               bits=np.full((NY, NX), 201, np.uint8), med=np.full((NY, NX), -77.0, np.float32),
               nmed=np.full((NY, NX), 201, np.uint8), minmed=np.full((NY, NX), 201, np.uint8))
    ft, wt, mt = de.pointer_table(frames, K), de.pointer_table(weights, K), de.pointer_table(masks, K)
    fn = lib.emuz_mm_minmed_f64 if np.dtype(dtype) == np.float64 else lib.emuz_mm_minmed_f32
    rc = fn(de._p(ft), de._p(wt), de._p(mt), de._p(shapes), de._p(maps), de._p(active), K, float(c['pixfrac']),
            ds.KERNELS[c['kernel']], p['nlow'], p['nhigh'], de._p(table), float(q['nsigma'][0]), float(q['nsigma'][1]),
            int(q['grow']), NY, NX, *[de._p(out[k]) for k in ('md', 'lo', 'bits', 'med', 'nmed', 'minmed')], grid)
    assert rc == 0, rc
    return out


def run_cr_grow(lib, c, dtype, k, med, nmed, seed, clean, g, cte, ctedir, grid=0):
    """(grown mask, clean) of frame k; `clean` (the seed pass's) is copied, not written"""
    frames, weights, masks, shapes, maps, active, K = de.arrays(c, dtype)
    NY, NX = c['out_shape']
    ny, nx = frames[k].shape
    crmask = np.full((ny, nx), 201, np.uint8)
    clean = np.array(clean, dtype, copy=True, order='C')
    seed = np.ascontiguousarray(seed, np.uint8)
    ft, wt, mt = de.pointer_table(frames, K), de.pointer_table(weights, K), de.pointer_table(masks, K)
    rs, rm = ce.rms_args(c, k, dtype)
    fn = lib.emuz_mm_cr_grow_f64 if np.dtype(dtype) == np.float64 else lib.emuz_mm_cr_grow_f32
    rc = fn(de._p(ft), de._p(wt), de._p(mt), de._p(shapes), de._p(maps), de._p(active), K, float(c['pixfrac']),
            ds.KERNELS[c['kernel']], k, de._p(med), de._p(nmed), NY, NX, rs, de._p(rm), de._p(seed), g, cte, ctedir,
            de._p(crmask), de._p(clean), grid)
    assert rc == 0, rc
    return crmask, clean


def blot_everywhere(lib, c, dtype, k, med, nmed):
    """the EXISTING comparison entry with snr = scale = (0, 0): it flags every testable pixel whose value differs
    from b and writes b there, so its `clean` is b on every testable pixel"""
    return ce.run_cr(lib, dict(c, cr=dict(c['cr'], snr=(0.0, 0.0), scale=(0.0, 0.0))), dtype, k, med, nmed)
