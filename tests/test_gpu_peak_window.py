"""Every kernel family on the MI355X with the correlation peak anywhere in the lag window: the cases of
tests/peak_cases.py, which tests/test_peak_window_cpu.py runs on CPU threads, through subpixal_amd.  The product's
dispatch picks the family from the shape; the eight-wave kernel of the 64 tile runs in a child process started with
SPX_PAIR64_WAVES=8 (the knob is read once per process)."""
import sys

import pytest

if 'peak_cases' not in sys.modules:
    pytest.register_assert_rewrite('peak_cases')
import peak_cases as pc                                                   # noqa: E402

pytestmark = pytest.mark.gpu
PAIR_FAMILIES = tuple(f for f in pc.FAMILIES if f != 'wave8')


@pytest.fixture(scope='module')
def backend():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return pc.GpuBackend()


def test_case_list_reaches_every_window_class_and_has_no_ties():
    assert pc.assert_no_ties() > 1000
    for family in pc.FAMILIES:
        pc.check_coverage(family)


@pytest.mark.parametrize('family,shape', [(f, s) for f in PAIR_FAMILIES for s in pc.FAMILIES[f]['shapes']],
                         ids=lambda v: v if isinstance(v, str) else '%dx%d' % v)
def test_swept_peak_vs_oracle(backend, family, shape):
    """one test per shape: every upsample and cc_type of it, the oracle computed once per cell"""
    for s, up, cc in pc.pair_cells(family):
        if s == shape:
            pc.check_pair_cell(backend, family, s, up, cc)


def test_eight_wave_kernel_swept_peak_and_batch():
    """the same cells and the batch checks on the eight-wave kernel, in a child process with its own time limit"""
    print(pc.run_family_in_child('wave8', {'SPX_PAIR64_WAVES': '8'}, timeout=300))


@pytest.mark.parametrize('kernel', tuple(pc.DISP5_SHAPES))
def test_reference_mode_swept_peak_vs_oracle(backend, kernel):
    for cc in ('CC', 'NCC', 'ZNCC'):
        for dtype in ('float32', 'float64'):
            pc.check_disp5(backend, kernel, cc, dtype)


@pytest.mark.parametrize('n', pc.BORDER_SIZES)
def test_peaks_on_the_window_border(backend, n):
    pc.check_borders(backend, n)


@pytest.mark.parametrize('family', PAIR_FAMILIES)
def test_batch_order_and_grid_stride(backend, family):
    pc.check_batch(backend, family)


def test_measured_figures_table(backend):
    """(last in the file, after every cell has run) the device column of profiles/r08/peak_window.txt: `pytest -s`
    prints it (the eight-wave kernel's rows are in its child's output); every figure is inside its
    tolerance"""
    print(pc.measured_table(backend, PAIR_FAMILIES))
