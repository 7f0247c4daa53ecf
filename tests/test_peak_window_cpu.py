"""Every kernel family with the correlation peak anywhere in the lag window, on CPU threads: the cases of
tests/peak_cases.py through the logic-check harness (tests/cpu_emu), each family forced with `tile=`.
tests/test_gpu_peak_window.py runs the same cases on the device.  The coverage tests prove, from a Python mirror
of each family's window arithmetic, that the case list reaches every form of it -- on a machine without a GPU."""
import sys

import pytest

if 'peak_cases' not in sys.modules:
    pytest.register_assert_rewrite('peak_cases')
import peak_cases as pc                                                   # noqa: E402

PAIR_FAMILIES = tuple(pc.FAMILIES)


@pytest.fixture(scope='module')
def backend():
    return pc.EmuBackend()


def _cell_id(c):
    return '%dx%d-u%d-%s' % (c[0][0], c[0][1], c[1], c[2])


def test_case_list_has_no_ties_and_fits_its_cutouts():
    assert pc.assert_no_ties() > 1000


@pytest.mark.parametrize('family', PAIR_FAMILIES)
def test_cases_reach_every_plane_wrap(family):
    for row in pc.check_coverage(family):
        print('%-8s %s %s' % row)


@pytest.mark.parametrize('family,cell', [(f, c) for f in PAIR_FAMILIES for c in pc.pair_cells(f)],
                         ids=lambda v: v if isinstance(v, str) else _cell_id(v))
def test_swept_peak_vs_oracle(backend, family, cell):
    pc.check_pair_cell(backend, family, *cell)


@pytest.mark.parametrize('dtype', ('float32', 'float64'))
@pytest.mark.parametrize('cc', ('CC', 'NCC', 'ZNCC'))
@pytest.mark.parametrize('kernel', tuple(pc.DISP5_SHAPES))
def test_reference_mode_swept_peak_vs_oracle(backend, kernel, cc, dtype):
    pc.check_disp5(backend, kernel, cc, dtype)


@pytest.mark.parametrize('n', pc.BORDER_SIZES)
def test_peaks_on_the_window_border(backend, n):
    pc.check_borders(backend, n)


@pytest.mark.parametrize('family', PAIR_FAMILIES)
def test_batch_order_and_grid_stride(backend, family):
    pc.check_batch(backend, family)


def test_measured_figures_table(backend):
    """(last in the file, after every cell has run) the CPU column of profiles/r08/peak_window.txt: `pytest -s`
    prints it for the cells
    that ran; every figure is inside its tolerance"""
    print(pc.measured_table(backend, PAIR_FAMILIES))
