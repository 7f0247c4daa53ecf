"""Deblending on the GPU (`subpixal_amd.detect.deblend`, `find_sources(deblend=True)`, spx_deblend_labels_*)
against the numpy/scipy statement of tests/deblend_statement.py: labels, parent and dflags with EXACT equality,
on the scenes of tests/deblend_cases.py that tests/test_deblend_cpu.py runs on the CPU harness.  Here the
kernels run as hipcc built them for gfx950, many workgroups at once, through LDS and through the workspace."""
import ctypes

import numpy as np
import pytest

import deblend_cases as dc
import deblend_statement as dst

pytestmark = pytest.mark.gpu
E_WORKSPACE = -4
_ST = {}


def _kw(s, over):
    kw = dict(levels_n=31, contrast=0.005, mode='exponential', min_area=5, conn=8)
    kw.update(s['kw'])
    kw.update(over)
    return kw


def statement(s, name, dtype, **over):
    key = (name, np.dtype(dtype).name, tuple(sorted(over.items())))
    if key not in _ST:
        kw = _kw(s, over)
        frame = np.ascontiguousarray(s['frame'], dtype)
        labels, n = dc.label_np(frame, s['thr'], s['mask'], s['filt'], kw['min_area'], kw['conn'])
        st = dst.statement(frame, labels, n, mask=s['mask'], filt=s['filt'], **kw)
        st['in_labels'], st['nparents'] = labels, n
        for a in st.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _ST[key] = st
    return _ST[key]


def run_deblend(s, st, dtype, **over):
    """detect.deblend on the statement's own input labels"""
    from subpixal_amd import detect
    kw = _kw(s, over)
    filt = None if s['filt'] is None else s['filt'].astype(dtype)
    lab, n, parent, dflags = detect.deblend(s['frame'].astype(dtype), np.array(st['in_labels']), st['nparents'],
                                            mask=s['mask'], filter_kernel=filt, levels=kw['levels_n'],
                                            contrast=kw['contrast'], mode=kw['mode'], min_area=kw['min_area'],
                                            connectivity=kw['conn'])
    return lab.cpu().numpy(), n, parent.cpu().numpy(), dflags.cpu().numpy()


def run_find(s, dtype, **over):
    from subpixal_amd import detect
    kw = _kw(s, over)
    filt = None if s['filt'] is None else s['filt'].astype(dtype)
    return detect.find_sources(s['frame'].astype(dtype), s['thr'], mask=s['mask'], filter_kernel=filt,
                               min_area=kw['min_area'], connectivity=kw['conn'], deblend=True,
                               deblend_levels=kw['levels_n'], deblend_contrast=kw['contrast'], deblend_mode=kw['mode'])


def both(s, name, dtype, **over):
    from subpixal_amd import detect
    st = statement(s, name, dtype, **over)
    dst.check(*run_deblend(s, st, dtype, **over), st, what=name + ' detect.deblend')
    src = run_find(s, dtype, **over)
    dst.check(src.segmentation.cpu().numpy(), len(src), src.parent, src.flags & 24, st, what=name + ' find_sources')
    # the measurements are those of the deblended segments
    assert np.array_equal(src.npix, np.bincount(st['labels'].ravel(), minlength=st['n'] + 1)[1:])
    assert src.table()['parent'] is src.parent and detect.FLAG_DEBLENDED == 8
    print('%s %s: %d parents -> %d segments' % (name, np.dtype(dtype).name, st['nparents'], st['n']))
    return st, src


SCENES = {'pair 6': lambda: dc.pair(6), 'pair 8': lambda: dc.pair(8), 'pair 12 0.1': lambda: dc.pair(12, 0.1),
          'pair 8 0.1': lambda: dc.pair(8, 0.1), 'triple': dc.triple, 'weak bump': dc.weak_bump,
          'late bloomer': dc.late_bloomer, 'plateaus': dc.plateaus, 'flat': dc.flat, 'needles': dc.needles,
          'corners': dc.corners, 'masked': dc.masked, 'ring': dc.ring, 'interleaved': dc.interleaved}


CASES = [(name, {}) for name in SCENES] + [('triple', dict(levels_n=7)), ('triple', dict(levels_n=1)),
                                           ('needles', dict(min_area=1)), ('ring', dict(conn=4))]
CASES += [('plateaus', dict(mode=m, conn=c)) for m in ('exponential', 'linear') for c in (8, 4)]


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('name,over', CASES, ids=['%s %s' % (n, ' '.join('%s=%s' % kv for kv in sorted(o.items())))
                                                  for n, o in CASES])
def test_scenes_against_the_statement(name, over, dtype):
    both(SCENES[name](), name, dtype, **over)


@pytest.mark.parametrize('mode', ['exponential', 'linear'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_lo_not_positive_takes_the_linear_levels(dtype, mode):
    s = dc.pair(12)
    st = statement(s, 'pair 12', dtype)
    shifted = dict(s, frame=s['frame'] - 8.0)
    frame = np.ascontiguousarray(shifted['frame'], dtype)
    ref = dst.statement(frame, np.array(st['in_labels']), st['nparents'], filt=s['filt'], mode=mode)
    lin = dst.statement(frame, np.array(st['in_labels']), st['nparents'], filt=s['filt'], mode='linear')
    assert np.array_equal(ref['labels'], lin['labels']) and ref['n'] == 2
    dst.check(*run_deblend(shifted, st, dtype, mode=mode), ref, what='shifted pair ' + mode)


@pytest.mark.parametrize('conn', [8, 4])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_smooth_random_field(dtype, conn):
    st, src = both(dc.smooth_field(), 'smooth field', dtype, conn=conn)
    assert st['nparents'] >= 10 and 3 <= len(st['split']) <= st['nparents'] // 2
    big, _ = both(dc.smooth_field(seed=12, shape=(240, 300)), 'smooth field 240x300', dtype, conn=conn)
    assert big['nparents'] >= 100 and len(big['split']) >= 20


def test_lds_path_against_workspace_path():
    """the 150 x 150 blob cannot fit LDS, the same blob at 40 x 40 does; both against the statement, and both
    give the same three children"""
    stb, _ = both(dc.blob(150), 'blob 150', np.float32)
    sts, _ = both(dc.blob(40), 'blob 40', np.float32)
    assert stb['n'] == sts['n'] == 3
    for st, lds in ((stb, False), (sts, True)):
        ys, xs = np.nonzero(st['in_labels'] == 1)
        assert ((np.ptp(ys) + 1) * (np.ptp(xs) + 1) <= 2048) == lds


def test_box_over_the_limit():
    from subpixal_amd import detect
    st, src = both(dc.big_ring(), 'big ring', np.float32)
    assert sorted(src.flags & 24) == [8, 8, detect.FLAG_NODEBLEND]
    assert np.array_equal(st['labels'] == 1, st['in_labels'] == 1)


def test_two_runs_are_bit_identical():
    s = dc.smooth_field(seed=12, shape=(240, 300))
    a, b = run_find(s, np.float32), run_find(s, np.float32)
    assert a.segmentation.cpu().numpy().tobytes() == b.segmentation.cpu().numpy().tobytes()
    assert a.table_device.cpu().numpy().tobytes() == b.table_device.cpu().numpy().tobytes()
    assert a.flags.tobytes() == b.flags.tobytes() and a.parent.tobytes() == b.parent.tobytes()


def test_deblend_off_is_bit_identical_to_plain_find_sources():
    from subpixal_amd import detect
    s = dc.smooth_field()
    f = s['frame'].astype(np.float32)
    a = detect.find_sources(f, s['thr'])
    b = detect.find_sources(f, s['thr'], deblend=False, deblend_levels=7, deblend_contrast=0.5, deblend_mode='linear')
    assert a.segmentation.cpu().numpy().tobytes() == b.segmentation.cpu().numpy().tobytes()
    assert a.table_device.cpu().numpy().tobytes() == b.table_device.cpu().numpy().tobytes()
    assert a.flags.tobytes() == b.flags.tobytes() and a.bbox.tobytes() == b.bbox.tobytes()
    assert a.parent is None and b.parent is None and 'parent' not in b.table()
    # and the labelling the deblended run starts from is that same image
    lab, n = detect.label(f, s['thr'])
    assert np.array_equal(lab.cpu().numpy(), statement(s, 'smooth field', np.float32)['in_labels']) and n == len(a)


def test_raw_call_with_a_short_workspace_writes_nothing():
    import torch
    from subpixal_amd import _ffi, cutout, device
    lib = _ffi.load()
    s = dc.interleaved()
    st = statement(s, 'interleaved', np.float32)
    ny, nx = s['frame'].shape
    f = torch.from_numpy(s['frame'].astype(np.float32)).cuda()
    k = torch.from_numpy(s['filt'].astype(np.float32)).cuda()
    seg = torch.from_numpy(np.array(st['in_labels'])).cuda()
    n = st['nparents']
    boxes, _ = cutout.segment_bounding_boxes(seg, max_label=n)
    need = lib.spx_deblend_workspace_bytes(ny, nx, n)
    work = torch.empty((need,), dtype=torch.uint8, device='cuda')
    out = torch.full((ny, nx), -3, dtype=torch.int32, device='cuda')
    tab = torch.full((2, 8), -3, dtype=torch.int32, device='cuda')
    nout = torch.full((1,), -3, dtype=torch.int32, device='cuda')

    def call(wb, max_out=8):
        return lib.spx_deblend_labels_f32(device.ptr(f), None, device.ptr(k), 3, 3, ny, nx, device.ptr(seg), n,
                                          device.ptr(boxes), 8, 5, 31, 0.005, 0, device.ptr(work), wb, device.ptr(out),
                                          device.ptr(tab[0]), device.ptr(tab[1]), max_out, device.ptr(nout),
                                          device.stream_ptr())
    assert call(need - 1) == E_WORKSPACE
    torch.cuda.synchronize()
    assert int(out.min()) == int(out.max()) == -3 and int(tab.max()) == -3 and int(nout.item()) == -3
    assert call(need, max_out=3) == 0
    torch.cuda.synchronize()
    assert int(nout.item()) == st['n'] == 4 and np.array_equal(out.cpu().numpy(), st['labels'])
    t = tab.cpu().numpy()
    assert np.array_equal(t[0, :3], st['parent'][:3]) and np.array_equal(t[1, :3], st['dflags'][:3])
    assert np.all(t[:, 3:] == -3)                      # rows beyond max_out are not written


def test_close_pairs_end_to_end():
    """N drawn close pairs that the statement splits: one catalog entry per drawn star, every drawn centre in a
    segment of its own.  No positional tolerance: the statement is the yardstick."""
    s = dc.crowded()
    st, src = both(s, 'crowded', np.float32)
    centres = s['centres']
    assert st['nparents'] == len(centres) // 2 and st['n'] == len(centres) and len(st['split']) == st['nparents']
    seg = src.segmentation.cpu().numpy()
    assert sorted(seg[y, x] for y, x in centres) == list(range(1, len(centres) + 1))
    cat = src.cutout_catalog(s['frame'].astype(np.float32))
    assert len(cat.src_id) == len(centres)
    assert sorted(int(i) for i in cat.src_id) == list(range(1, len(centres) + 1))
