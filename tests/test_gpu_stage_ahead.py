"""On the device: a pair's result does not depend on whether its predecessor staged it (spx_kernels.h pair_body;
tests/test_stage_ahead_cpu.py has the same property on CPU threads).  One call with a batch of twice the launched
grid plus 37 pairs -- every workgroup walks 2-3 pairs, all but the first of a walk staged by the pair before --
against the same pairs sent in chunks no larger than the grid, where every workgroup has one pair and stages it
itself.  Equality, not a tolerance: both ways are the same operations on the same values."""
import numpy as np
import pytest

import emu
from oracle import subpixal_oracle as orc

pytestmark = pytest.mark.gpu

UP = 10
ST_NONFINITE = 6


@pytest.fixture(scope='module')
def batch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import subpixal_amd as spx
    from subpixal_amd import synth
    grid = 32 * torch.cuda.get_device_properties(0).multi_processor_count      # spx_capi.hip grid_for
    count = 2 * grid + 37
    ref, img, truth = synth.gaussian_pairs(count, 64)
    # workgroup b walks the items first_item(b) + k * grid: three of the 37 workgroups that walk three pairs get a
    # NaN pixel in their first, their middle and their last pair
    firsts = [emu.first_item(b, grid) for b in (1, 3, 4)]
    assert len(set(firsts)) == 3 and all(0 <= j < 37 for j in firsts), firsts
    bad = [firsts[0], firsts[1] + grid, firsts[2] + 2 * grid]
    img[bad[0], 17, 23] = float('nan')
    ref[bad[1], 40, 5] = float('nan')
    img[bad[2], 0, 63] = float('nan')
    return dict(spx=spx, grid=grid, count=count, ref=ref, img=img, truth=truth, bad=bad)


def test_walked_batch_equals_chunks_of_one_pair_per_workgroup(batch):
    import torch
    spx, grid, count, ref, img = (batch[k] for k in ('spx', 'grid', 'count', 'ref', 'img'))
    got, st = spx.xcorr_refine_batch(ref, img, upsample=UP, return_status=True)
    parts = [spx.xcorr_refine_batch(ref[a:a + grid], img[a:a + grid], upsample=UP, return_status=True)
             for a in range(0, count, grid)]
    exp, est = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    assert torch.equal(st, est)
    assert torch.equal(got.view(torch.int64), exp.view(torch.int64))
    finite = torch.ones(count, dtype=torch.bool, device=got.device)
    finite[batch['bad']] = False
    assert torch.all(st[batch['bad']] == ST_NONFINITE) and torch.all(st[finite] == 0)
    err = float((got - batch['truth'])[finite].abs().max())
    assert err < 1e-3, err
    # and the same call again: bit for bit
    again, st2 = spx.xcorr_refine_batch(ref, img, upsample=UP, return_status=True)
    assert torch.equal(again.view(torch.int64), got.view(torch.int64)) and torch.equal(st2, st)


def test_normalised_correlation_still_takes_its_own_path(batch):
    """NCC needs the successor's statistics before its pixels: no stage-ahead.  16 sampled pairs against the oracle"""
    spx, count, ref, img = (batch[k] for k in ('spx', 'count', 'ref', 'img'))
    got, st = spx.xcorr_refine_batch(ref, img, upsample=UP, cc_type='NCC', return_status=True)
    pick = [int(p) for p in np.linspace(0, count - 1, 16).astype(np.int64) if int(p) not in batch['bad']]
    assert len(pick) >= 14
    exp, est = orc.xcorr_refine_batch(ref[pick].cpu().numpy(), img[pick].cpu().numpy(), UP, 'NCC')
    assert np.array_equal(st[pick].cpu().numpy(), est)
    err = float(np.max(np.abs(got[pick].cpu().numpy() - exp)))
    assert err < 2e-4, err            # tests/test_gpu_parity.py: float32 refine at upsample 10
