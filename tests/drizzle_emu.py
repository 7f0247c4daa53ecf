"""The drizzle kernel on CPU threads for the tests: builds tests/cpu_emu/emu_drizzle.cpp on the fly with the Makefile's
emu compiler and flags (as test_errors_cpu.py builds its harness) and runs a case of drizzle_cases.py through it.
Not a test module.  SPX_EMU_DRIZZLE_LIB: a pre-built harness."""
import ctypes
import os
import subprocess

import numpy as np

import drizzle_statement as ds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'subpixal_amd', 'csrc')
_LIB = {}
_vp, _int, _dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double


def load(tmp_path_factory):
    if 'lib' not in _LIB:
        so = os.environ.get('SPX_EMU_DRIZZLE_LIB')
        if not so:
            out = subprocess.check_output(['make', '-s', '-C', CSRC, '--eval',
                                           'spx-emu-flags: ; @echo $(HOSTCXX) $(EMUFLAGS)', 'spx-emu-flags'],
                                          universal_newlines=True).split()
            so = str(tmp_path_factory.mktemp('emuz') / 'libspx_emu_drizzle.so')
            subprocess.check_call(out + ['-shared', '-o', so, os.path.join(ROOT, 'tests', 'cpu_emu', 'emu_drizzle.cpp')])
        lib = ctypes.CDLL(so)
        for fn in (lib.emuz_drizzle_f32, lib.emuz_drizzle_f64):
            fn.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _int, _dbl, _int, _dbl, _int, _int, _vp, _vp, _vp, _int]
        _LIB['lib'] = lib
    return _LIB['lib']


def arrays(c, dtype):
    """the case's frames, weights and masks as contiguous arrays of `dtype` / uint8 (None stays None)"""
    frames = [np.ascontiguousarray(f, dtype) for f in c['frames']]
    K = len(frames)
    weights = None if c['weights'] is None else [None if w is None else np.ascontiguousarray(w, dtype)
                                                 for w in c['weights']]
    masks = None if c['masks'] is None else [None if m is None else np.ascontiguousarray(m, np.uint8)
                                             for m in c['masks']]
    shapes = np.array([f.shape for f in frames], np.int32)
    maps = np.ascontiguousarray(np.stack(c['maps']), np.float64)
    active = None if c['active'] is None else np.asarray(c['active'], np.uint8)
    return frames, weights, masks, shapes, maps, active, K


def pointer_table(arrs, K):
    if arrs is None:
        return None
    return np.array([0 if a is None else a.ctypes.data for a in arrs], np.uint64)


def _p(a):
    return None if a is None else a.ctypes.data_as(_vp)


def run(lib, c, dtype, grid=0, expect=0):
    frames, weights, masks, shapes, maps, active, K = arrays(c, dtype)
    NY, NX = c['out_shape']
    sci = np.full((NY, NX), -77.0, dtype)
    wht = np.full((NY, NX), -77.0, np.float32)
    ctx = np.full(((K + 31) // 32, NY, NX), -77, np.int32)
    ft, wt, mt = pointer_table(frames, K), pointer_table(weights, K), pointer_table(masks, K)
    fn = lib.emuz_drizzle_f64 if np.dtype(dtype) == np.float64 else lib.emuz_drizzle_f32
    rc = fn(_p(ft), _p(wt), _p(mt), _p(shapes), _p(maps), _p(active), K, float(c['pixfrac']),
            ds.KERNELS[c['kernel']], float(c['fill']), NY, NX, _p(sci), _p(wht), _p(ctx), grid)
    assert rc == expect, rc
    return sci, wht, ctx


_ST = {}


def statement(name, c):
    """the statement of a named case, computed once and shared (read-only) by every test that needs it"""
    if name not in _ST:
        st = ds.statement(c['frames'], c['maps'], c['out_shape'], weights=c['weights'], masks=c['masks'],
                          active=c['active'], pixfrac=c['pixfrac'], kernel=c['kernel'], fill=c['fill'])
        for v in st.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _ST[name] = st
    return _ST[name]
