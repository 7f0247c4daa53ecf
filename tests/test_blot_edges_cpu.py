"""The dithered-blot kernels at source edges, on small sources and at every polynomial degree, on CPU threads
(tests/emu.py runs the source hipcc compiles): the cases of tests/blot_cases.py, which
tests/test_gpu_blot_edges.py runs on the MI355X.  What is held: agreement with the interpolant and the edge
continuation the header comment above everett5 states, against the oracle's independent float64 Lagrange form
-- not parity with drizzlepac."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import emu

if 'blot_cases' not in sys.modules:
    pytest.register_assert_rewrite('blot_cases')
import blot_cases as bc                                                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'subpixal_amd', 'csrc')
_LIB = {}


def _emu64(tmp_path_factory):
    """tests/cpu_emu/emu_catalog_f64.cpp (the emu64_blot4_var_* entries) built with the Makefile's emu compiler
    and flags, as tests/test_catalog_f64_cpu.py builds it"""
    if 'lib' not in _LIB:
        out = subprocess.check_output(['make', '-s', '-C', CSRC, '--eval',
                                       'spx-emu-flags: ; @echo $(HOSTCXX) $(EMUFLAGS)', 'spx-emu-flags'],
                                      universal_newlines=True).split()
        so = str(tmp_path_factory.mktemp('emu64_blot') / 'libspx_emu_catalog_f64.so')
        subprocess.check_call(out + ['-shared', '-o', so, os.path.join(ROOT, 'tests', 'cpu_emu',
                                                                      'emu_catalog_f64.cpp')])
        _LIB['lib'] = ctypes.CDLL(so)
    return _LIB['lib']


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class EmuBackend:
    def __init__(self, lib64):
        self.lib64 = lib64

    def affine(self, src, aff, shape, gain=None):
        return emu.blot_affine4(src, aff, shape[0], shape[1], gain)

    def poly(self, src, coef, degree, shape, gain=None):
        return emu.blot_poly4(src, coef, degree, shape[0], shape[1], gain)

    def packed(self, src, soffs, sshapes, maps, degree, doffs, dshapes, out, gain=None):
        """float32: the main harness's entry and the float64 harness's float32 one, which must agree"""
        args = (_ptr(src), _ptr(soffs), _ptr(sshapes), ctypes.c_int64(len(soffs)), _ptr(maps), int(degree),
                _ptr(None if gain is None else np.ascontiguousarray(gain, np.float32)), _ptr(doffs), _ptr(dshapes))
        if out.dtype == np.float64:
            assert self.lib64.emu64_blot4_var_to_f64(*args, _ptr(out)) == 0
            return out
        twin = out.copy()
        assert emu.lib().emu_blot4_var(*args, _ptr(out)) == 0
        assert self.lib64.emu64_blot4_var_f32(*args, _ptr(twin)) == 0
        assert np.array_equal(out, twin, equal_nan=True)
        return out


@pytest.fixture(scope='module')
def backend(tmp_path_factory):
    return EmuBackend(_emu64(tmp_path_factory))


def test_case_module_restates_the_oracle_and_reaches_every_band_class():
    for case in bc.group1()[:2] + bc.group3()[:3] + bc.group7()[:1]:
        bc.check_restates_oracle(case)
    bc.check_group3_coverage()
    for cases in (bc.group1(), bc.group7(), tuple(bc.group4().values())):
        assert sum(c.pixels for c in cases) <= 20000                      # the oracle is Python loops


@pytest.mark.parametrize('kernel', bc.KERNELS)
def test_integer_translations_copy_the_source(backend, kernel):
    bc.check_group1(backend, kernel)


@pytest.mark.parametrize('kernel', bc.KERNELS)
def test_integer_ramps_are_exact_in_every_cell(backend, kernel):
    bc.check_group2(backend, kernel)


@pytest.mark.parametrize('shape', bc.G3_SHAPES, ids=lambda s: '%dx%d' % s)
@pytest.mark.parametrize('kernel', bc.KERNELS)
def test_every_band_position_vs_float64_oracle(backend, kernel, shape):
    bc.check_group3(backend, kernel, shape)


@pytest.mark.parametrize('degree', (1, 2, 3, 4, 5))
def test_every_polynomial_degree_and_unused_slots(backend, degree):
    bc.check_group4(backend, degree)


@pytest.mark.parametrize('degree', (0, 3))
def test_packed_mixed_shapes_equal_fixed_shape_kernels(backend, degree):
    bc.check_group5(backend, degree)


def test_grid_stride_of_the_fixed_shape_kernels(backend):
    """12 sources of 6x6 onto 8x8 = 12 workgroups of output on a grid of 2: six passes"""
    emu.set_grid(2)
    try:
        picks = bc.check_grid_stride(backend, 12, (6, 6), (8, 8), 2 * 256)
    finally:
        emu.set_grid(0)
    assert len(picks) == 12


@pytest.mark.parametrize('kernel', bc.KERNELS)
def test_nan_sample_stays_local(backend, kernel):
    bc.check_group7(backend, kernel)
