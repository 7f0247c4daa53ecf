"""The dithered-blot kernels on the MI355X at source edges, on small sources and at every polynomial degree
(spx_blot_affine4_f32, spx_blot_poly4_f32, spx_blot4_var_f32, spx_blot4_var_to_f64): the cases of
tests/blot_cases.py, which tests/test_blot_edges_cpu.py runs on CPU threads.  What is held: agreement with the
interpolant and the edge continuation the header comment above everett5 states, against the oracle's
independent float64 Lagrange form -- not parity with drizzlepac."""
import sys

import numpy as np
import pytest

if 'blot_cases' not in sys.modules:
    pytest.register_assert_rewrite('blot_cases')
import blot_cases as bc                                                   # noqa: E402

pytestmark = pytest.mark.gpu


class GpuBackend:
    def affine(self, src, aff, shape, gain=None):
        from subpixal_amd import blot
        return blot.blot_affine4_batch(src, aff, shape, gain)

    def poly(self, src, coef, degree, shape, gain=None):
        from subpixal_amd import blot
        return blot.blot_poly4_batch(src, coef, shape, degree, gain)

    def packed(self, src, soffs, sshapes, maps, degree, doffs, dshapes, out, gain=None):
        """The C entry on a test-owned tensor that holds `out` (its sentinels between the items included), so
        the guard elements are memory this test allocated; then blot.blot4_packed, which allocates its own
        buffer of the same layout, must give the same items."""
        import torch
        from subpixal_amd import _ffi, blot, device
        dev = 'cuda:%d' % device.init()
        t = [torch.as_tensor(np.ascontiguousarray(a)).to(dev) for a in (src, soffs, sshapes, maps, doffs, dshapes)]
        g = None if gain is None else torch.as_tensor(np.ascontiguousarray(gain, np.float32)).to(dev)
        im4 = torch.as_tensor(out).to(dev)
        lib = _ffi.load()
        fn = lib.spx_blot4_var_to_f64 if out.dtype == np.float64 else lib.spx_blot4_var_f32
        with torch.cuda.device(im4.device):
            _ffi.check(fn(device.ptr(t[0]), device.ptr(t[1]), device.ptr(t[2]), len(soffs), device.ptr(t[3]),
                          int(degree), device.ptr(g), device.ptr(t[4]), device.ptr(t[5]), device.ptr(im4),
                          device.stream_ptr()))
        got = im4.cpu().numpy()
        own = blot.blot4_packed(t[0], t[1], t[2], t[3], t[4], t[5], out.size // 4, degree, g, im4.dtype).cpu().numpy()
        assert own.shape == got.shape and own.dtype == got.dtype
        for (h, w), o in zip(dshapes, doffs):
            item = slice(4 * int(o), 4 * int(o) + 4 * int(h) * int(w))
            assert np.array_equal(own[item], got[item], equal_nan=True)
        return got


@pytest.fixture(scope='module')
def backend():
    return GpuBackend()


def test_case_module_reaches_every_band_class():
    bc.check_group3_coverage()


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
    """The host caps the grid at 65536 workgroups of 256: 4200 sources of 16x16 onto 32x32 are 17.2 M output
    elements, 0.4 M more than one pass of that grid covers; the boundary lies between items 4095 and 4096."""
    picks = bc.check_grid_stride(backend, 4200, (16, 16), (32, 32), 65536 * 256)
    assert {0, 4095, 4096, 4097, 4199} <= set(picks.tolist()) and len(picks) == 64


@pytest.mark.parametrize('kernel', bc.KERNELS)
def test_nan_sample_stays_local(backend, kernel):
    bc.check_group7(backend, kernel)
