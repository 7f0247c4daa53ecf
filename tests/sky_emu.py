"""The whole-frame statistics kernels on CPU threads for the tests: builds tests/cpu_emu/emu_sky.cpp on the fly with
the Makefile's emu compiler and flags (as crreject_emu.py builds its harness) and runs a case of sky_cases.py through
it.  Not a test module.  SPX_EMU_SKY_LIB: a pre-built harness."""
import ctypes
import os
import subprocess

import numpy as np

import sky_statement as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'subpixal_amd', 'csrc')
_LIB = {}
_vp, _int, _dbl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
COLUMNS = ('sky', 'med', 'mean', 'std', 'lo', 'hi')


def emu_flags():
    return subprocess.check_output(['make', '-s', '-C', CSRC, '--eval',
                                    'spx-emu-flags: ; @echo $(HOSTCXX) $(EMUFLAGS)', 'spx-emu-flags'],
                                   universal_newlines=True).split()


def load(tmp_path_factory):
    if 'lib' not in _LIB:
        so = os.environ.get('SPX_EMU_SKY_LIB')
        if not so:
            so = str(tmp_path_factory.mktemp('emus') / 'libspx_emu_sky.so')
            subprocess.check_call(emu_flags() + ['-shared', '-o', so, os.path.join(ROOT, 'tests', 'cpu_emu', 'emu_sky.cpp')])
        lib = ctypes.CDLL(so)
        for fn in (lib.emus_sky_stats_f32, lib.emus_sky_stats_f64):
            fn.argtypes = [_vp, _vp, _vp, _vp, _int, _dbl, _dbl, _dbl, _dbl, _int, _int, _vp, _vp, _vp, _int]
        _LIB['lib'] = lib
    return _LIB['lib']


def _p(a):
    return None if a is None else a.ctypes.data_as(_vp)


def table(arrays):
    return np.array([0 if a is None else a.ctypes.data for a in arrays], np.uint64)


def prepared(c, dtype):
    """contiguous arrays of a case: frames and weights in `dtype`, masks uint8"""
    K = len(c['frames'])
    frames = [np.ascontiguousarray(f, dtype) for f in c['frames']]
    weights = None if c['weights'] is None else [None if w is None else np.ascontiguousarray(w, dtype)
                                                 for w in c['weights']]
    masks = None if c['masks'] is None else [None if m is None else np.ascontiguousarray(m, np.uint8)
                                             for m in c['masks']]
    return frames, weights, masks, K


def rows(out, counts, status):
    """per frame a dict of the kernel's results"""
    res = []
    for k in range(out.shape[0]):
        d = {n: float(out[k, i]) for i, n in enumerate(COLUMNS)}
        d.update(n_usable=int(counts[k, 0]), n_final=int(counts[k, 1]), status=int(status[k, 0]),
                 rounds=int(status[k, 1]))
        res.append(d)
    return res


def run(lib, c, dtype, gpf=1, frames_only=None):
    """(rows, raw bytes of the three tables) of a case on CPU threads; `frames_only`: a list of frame indices"""
    frames, weights, masks, K = prepared(c, dtype)
    idx = list(range(K)) if frames_only is None else list(frames_only)
    frames = [frames[k] for k in idx]
    weights = None if weights is None else [weights[k] for k in idx]
    masks = None if masks is None else [masks[k] for k in idx]
    K = len(idx)
    ft = table(frames)
    wt = None if weights is None else table(weights)
    mt = None if masks is None else table(masks)
    shapes = np.array([f.shape for f in frames], np.int32)
    out = np.full((K, 6), -77.0)
    counts = np.full((K, 2), -77, np.int64)
    status = np.full((K, 2), -77, np.int32)
    nan = float('nan')
    fn = lib.emus_sky_stats_f64 if np.dtype(dtype) == np.float64 else lib.emus_sky_stats_f32
    rc = fn(_p(ft), _p(wt), _p(mt), _p(shapes), K, nan if c['lower'] is None else c['lower'],
            nan if c['upper'] is None else c['upper'], c['lsigma'], c['usigma'], c['max_iters'],
            ss.STATS[c['stat']], _p(out), _p(counts), _p(status), gpf)
    assert rc == 0, rc
    return rows(out, counts, status), out.tobytes() + counts.tobytes() + status.tobytes()


_ST = {}


def statements(name, c, dtype):
    """the statement of every frame of a named case and dtype, computed once and shared (read-only)"""
    key = (name, np.dtype(dtype).name)
    if key not in _ST:
        frames, weights, masks, K = prepared(c, dtype)
        _ST[key] = [ss.statement(frames[k], None if weights is None else weights[k],
                                 None if masks is None else masks[k], c['lower'], c['upper'], c['lsigma'],
                                 c['usigma'], c['max_iters'], c['stat']) for k in range(K)]
    return _ST[key]
