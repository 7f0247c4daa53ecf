"""The polynomial-map drizzle kernel on CPU threads for the tests: builds tests/cpu_emu/emu_drizzle_poly.cpp on the fly
with the Makefile's emu compiler and flags (as drizzle_emu.py does) and runs a case of drizzle_poly_cases.py through
it.  Not a test module.  SPX_EMU_DRIZZLE_POLY_LIB: a pre-built harness."""
import ctypes
import os
import subprocess

import numpy as np

import drizzle_emu as de
import drizzle_poly_statement as dps

ROOT = de.ROOT
_LIB = {}
_vp, _int, _dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
_p, pointer_table = de._p, de.pointer_table


def load(tmp_path_factory):
    if 'lib' not in _LIB:
        so = os.environ.get('SPX_EMU_DRIZZLE_POLY_LIB')
        if not so:
            out = subprocess.check_output(['make', '-s', '-C', de.CSRC, '--eval',
                                           'spx-emu-flags: ; @echo $(HOSTCXX) $(EMUFLAGS)', 'spx-emu-flags'],
                                          universal_newlines=True).split()
            so = str(tmp_path_factory.mktemp('emuzp') / 'libspx_emu_drizzle_poly.so')
            subprocess.check_call(out + ['-shared', '-o', so,
                                         os.path.join(ROOT, 'tests', 'cpu_emu', 'emu_drizzle_poly.cpp')])
        lib = ctypes.CDLL(so)
        for fn in (lib.emuz_drizzle_poly_f32, lib.emuz_drizzle_poly_f64):
            fn.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _int, _dbl, _int, _dbl, _int, _int, _vp, _vp, _vp,
                           _int]
        _LIB['lib'] = lib
    return _LIB['lib']


def map_tables(maps):
    """coef [K][2][21], degree [K], center [K][2] of a list of [6] arrays and PolyMaps"""
    pm = [dps.as_poly(m) for m in maps]
    return (np.ascontiguousarray(np.stack([m.coef for m in pm])), np.array([m.degree for m in pm], np.int32),
            np.ascontiguousarray(np.stack([m.center for m in pm])))


def arrays(c, dtype):
    """the case's frames, weights and masks as contiguous arrays of `dtype` / uint8 (None stays None)"""
    frames, weights, masks, shapes, _, active, K = de.arrays(dict(c, maps=[np.zeros(6) for _ in c['maps']]), dtype)
    return frames, weights, masks, shapes, active, K


def run(lib, c, dtype, grid=0, expect=0, sentinel=-77.0, guard=0):
    """the outputs of the harness; with ``guard`` rows of sentinel before and after each output in the same
    allocation, which are checked to be untouched"""
    frames, weights, masks, shapes, active, K = arrays(c, dtype)
    coef, degree, center = map_tables(c['maps'])
    NY, NX = c['out_shape']
    P = (K + 31) // 32
    full = [np.full((NY + 2 * guard, NX), sentinel, dtype), np.full((NY + 2 * guard, NX), sentinel, np.float32),
            np.full((P * NY + 2 * guard, NX), int(sentinel), np.int32)]
    sci, wht = full[0][guard:guard + NY], full[1][guard:guard + NY]
    ctx = full[2][guard:guard + P * NY].reshape(P, NY, NX)
    ft, wt, mt = pointer_table(frames, K), pointer_table(weights, K), pointer_table(masks, K)
    fn = lib.emuz_drizzle_poly_f64 if np.dtype(dtype) == np.float64 else lib.emuz_drizzle_poly_f32
    rc = fn(_p(ft), _p(wt), _p(mt), _p(shapes), _p(coef), _p(degree), _p(center), _p(active), K, float(c['pixfrac']),
            dps.KERNELS[c['kernel']], float(c['fill']), NY, NX, _p(sci), _p(wht), _p(ctx), grid)
    assert rc == expect, rc
    for f in full:
        assert np.all(f[:guard] == f.dtype.type(sentinel)) and np.all(f[f.shape[0] - guard:] == f.dtype.type(sentinel))
    return sci, wht, ctx


_ST = {}


def statement(name, c):
    """the statement of a named case, computed once and shared (read-only) by every test that needs it"""
    if name not in _ST:
        st = dps.statement(c['frames'], c['maps'], c['out_shape'], weights=c['weights'], masks=c['masks'],
                           active=c['active'], pixfrac=c['pixfrac'], kernel=c['kernel'], fill=c['fill'])
        for v in st.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _ST[name] = st
    return _ST[name]


def pack_rows(c, lib=None):
    """(rc, rows uint8 [K][ROW_BYTES]) of the library's own host entry for the case (no device needed: the frame
    pointers are host addresses, which the packing only stores)"""
    from subpixal_amd import _ffi
    lib = lib or _ffi.load()
    frames, weights, masks, shapes, active, K = arrays(c, np.float32)
    coef, degree, center = map_tables(c['maps'])
    ft = pointer_table(frames, K)
    rows = np.zeros((K, _ffi.DRIZZLE_POLY_ROW_BYTES), np.uint8)
    NY, NX = c['out_shape']
    rc = lib.spx_drizzle_poly_rows(ft.ctypes.data, None, None, shapes.ctypes.data, coef.ctypes.data,
                                   degree.ctypes.data, center.ctypes.data, None, K, float(c['pixfrac']),
                                   dps.KERNELS[c['kernel']], NY, NX, rows.ctypes.data)
    return rc, rows


def window(row):
    """(rx, ry) of a packed row"""
    from subpixal_amd import _ffi
    return tuple(row[_ffi.DRIZZLE_POLY_ROW_WINDOW:_ffi.DRIZZLE_POLY_ROW_WINDOW + 16].view(np.float64))
