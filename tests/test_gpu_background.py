"""Background estimation on the GPU (`subpixal_amd.detect.estimate_background` / `detect_sources`,
spx_background_mesh_* / spx_background_maps_*) against the numpy/scipy statement of tests/background_statement.py,
on the cases of tests/test_background_cpu.py (tests/background_cases.py); run-to-run bit identity; the C entries
through raw pointers; detection end to end without being given the background."""
import ctypes

import numpy as np
import pytest

import background_cases as bc
import background_statement as bs

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


def run(frame, box, filter_size=3, mask=None, exclude=None, sigma=3.0, max_iters=10, min_good_fraction=0.5,
        nsigma=2.5):
    from subpixal_amd import _ffi, detect
    try:
        bg = detect.estimate_background(frame, box=box, filter_size=filter_size, mask=mask, exclude=exclude,
                                        sigma=sigma, max_iters=max_iters, min_good_fraction=min_good_fraction)
    except _ffi.SubpixalHipError as e:
        assert 'no good cell' in str(e)
        raise bs.NoGoodCell()
    assert bg.background.is_cuda and bg.rms.is_cuda and bg.background.shape == frame.shape
    thr = bg.threshold(nsigma)
    assert thr.is_cuda and thr.dtype == torch.float32
    return dict(mesh_bkg=bg.mesh_background_raw, mesh_rms=bg.mesh_rms_raw, ngood=bg.mesh_ngood,
                filt_bkg=bg.mesh_background, filt_rms=bg.mesh_rms, bkg=bg.background.cpu().numpy(),
                rms=bg.rms.cpu().numpy(), thr=thr.cpu().numpy())


@pytest.mark.parametrize('name,shape,box,dtype', bc.GEOMETRY)
def test_mesh_geometry(name, shape, box, dtype):
    f = bc.sky(shape, 3, dtype)
    st, got = bc.check_case(run, f, box, '%s %s' % (name, np.dtype(dtype)))
    if name == 'one cell':
        assert np.all(got['bkg'] == got['bkg'][0, 0]) and np.all(got['rms'] == got['rms'][0, 0])
    if name == 'one knot in y':
        assert np.array_equal(got['bkg'], np.repeat(got['bkg'][:1], shape[0], axis=0))
    if name == 'two knots':
        inner = got['bkg'].astype(np.float64)[32:95, 32:95]
        assert np.abs(np.diff(inner, 2, axis=0)).max() <= 8 * np.finfo(dtype).eps * np.abs(inner).max()


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_blob_constant_and_max_iters(dtype):
    st, got = bc.check_case(run, bc.blob_scene(dtype), (32, 32), 'blob %s' % np.dtype(dtype))
    bc.check_blob_cell(st, got)
    st0, got0 = bc.check_case(run, bc.blob_scene(dtype), (32, 32), 'blob, max_iters=0', max_iters=0)
    assert got0['mesh_rms'][1, 1] > 5 * got['mesh_rms'][1, 1]
    bc.check_case(run, bc.blob_scene(dtype), (32, 32), 'blob, max_iters=40', max_iters=40)
    f = np.full((50, 70), 3.25, dtype)
    st, got = bc.check_case(run, f, (16, 24), 'constant')
    assert np.all(got['bkg'] == 3.25) and np.all(got['rms'] == 0) and np.all(got['thr'] == 3.25)


@pytest.mark.parametrize('fs', [1, 3, 5])
def test_filter_sizes(fs):
    f = bc.with_blob(bc.sky((150, 203), 6, np.float32), 70.0, 100.0, amp=80.0, sig=20.0)
    st, got = bc.check_case(run, f, (32, 48), 'filter %d' % fs, filter_size=fs)
    assert np.array_equal(got['filt_bkg'], got['mesh_bkg']) == (fs == 1)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_bad_pixels_mask_exclude_and_clamped_rms(dtype):
    rng = np.random.default_rng(7)
    f = bc.sky((100, 130), 8, dtype)
    f[rng.random(f.shape) < 0.01] = np.nan
    f[rng.random(f.shape) < 0.005] = np.inf
    f[rng.random(f.shape) < 0.005] = -np.inf
    mask = rng.random(f.shape) < 0.05
    mask[32:64, 48:96] = True
    st, got = bc.check_case(run, f, (32, 48), 'bad data', mask=mask)
    assert st['mesh']['ngood'][1, 1] == 0 and np.isnan(got['mesh_bkg'][1, 1]) and np.isfinite(got['filt_bkg'][1, 1])
    labels = np.zeros(f.shape, np.int32)
    labels[10:30, 10:40] = 3
    labels[70:75, 100:130] = 9
    g = bc.with_blob(f, 20.0, 25.0, amp=500.0, sig=5.0)
    bc.check_case(run, g, (32, 48), 'exclude', mask=mask, exclude=labels)

    def run_resident(frame, box, mask=None, exclude=None, **kw):     # the statement keeps the host copies
        return run(torch.from_numpy(frame).cuda(), box, mask=torch.from_numpy(mask).cuda(),
                   exclude=torch.from_numpy(exclude).cuda(), **kw)
    bc.check_case(run_resident, g, (32, 48), 'exclude, device frame, mask and labels', mask=mask, exclude=labels)
    u = bc.undershoot_scene(dtype)
    st, got = bc.check_case(run, u, (8, 8), 'undershoot', filter_size=1)
    assert bs.expand(st['filt_rms'], u.shape, (8, 8)).min() < -1e-3 and got['rms'].min() == 0.0


def test_isolated_good_cell_and_no_good_cell():
    f = bc.sky((64, 80), 9, np.float32)
    mask = np.ones(f.shape, bool)
    mask[0:16, 0:16] = False
    st, got = bc.check_case(run, f, (16, 16), 'isolated good cell', mask=mask)
    assert np.all(got['filt_bkg'] == got['mesh_bkg'][0, 0]) and np.all(got['filt_rms'] == got['mesh_rms'][0, 0])
    mask[48:64, 64:80] = False
    st, got = bc.check_case(run, f, (16, 16), 'two good cells', mask=mask)
    assert got['filt_bkg'][1, 2] == 0.5 * (got['mesh_bkg'][0, 0] + got['mesh_bkg'][3, 4])
    with pytest.raises(bs.NoGoodCell):
        run(f, (16, 16), mask=np.ones(f.shape, bool))


def test_bit_identical_from_run_to_run_and_on_a_side_stream():
    f = torch.from_numpy(bc.with_blob(bc.sky((300, 420), 12, np.float32), 100.0, 200.0)).cuda()
    a = run(f, (32, 48))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = run(f, (32, 48))
    side.synchronize()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_c_abi_through_raw_pointers():
    from subpixal_amd import _ffi
    lib = _ffi.load()
    assert lib.spx_abi_version() == 4
    vp = ctypes.c_void_p
    fh = bc.sky((100, 130), 13, np.float32)
    f = torch.from_numpy(fh).cuda()
    ny, nx, bh, bw, ncy, ncx = 100, 130, 32, 48, 4, 3
    mb = torch.full((ncy, ncx), -5.0, dtype=torch.float64, device='cuda')
    mr, ng = mb.clone(), torch.full((ncy, ncx), -5, dtype=torch.int32, device='cuda')
    s = torch.cuda.current_stream().cuda_stream
    assert lib.spx_background_mesh_f32(vp(f.data_ptr()), None, None, ny, nx, 4, bw, 3.0, 10, 0.5, vp(mb.data_ptr()),
                                       vp(mr.data_ptr()), vp(ng.data_ptr()), s) == -2
    assert lib.spx_background_mesh_f32(vp(f.data_ptr()), None, None, ny, nx, 128, 129, 3.0, 10, 0.5,
                                       vp(mb.data_ptr()), vp(mr.data_ptr()), vp(ng.data_ptr()), s) == -2
    torch.cuda.synchronize()
    assert float(mb.min()) == -5.0                      # a refused call writes nothing
    assert lib.spx_background_mesh_f32(vp(f.data_ptr()), None, None, ny, nx, bh, bw, 3.0, 10, 0.5, vp(mb.data_ptr()),
                                       vp(mr.data_ptr()), vp(ng.data_ptr()), s) == 0
    need = lib.spx_background_workspace_bytes(ny, nx, bh, bw)
    work = torch.zeros(need, dtype=torch.uint8, device='cuda')
    bkg = torch.full((ny, nx), -5.0, dtype=torch.float32, device='cuda')
    rms, thr = bkg.clone(), bkg.clone()
    status = torch.full((1,), -5, dtype=torch.int32, device='cuda')

    def maps(wb, o):
        return lib.spx_background_maps_f32(vp(mb.data_ptr()), vp(mr.data_ptr()), vp(ng.data_ptr()), ncy, ncx, bh, bw, 3,
                                           ny, nx, 2.5, vp(work.data_ptr()), wb, o[0], o[1], o[2],
                                           vp(status.data_ptr()), s)
    assert maps(need - 1, (vp(bkg.data_ptr()), None, None)) == -4
    torch.cuda.synchronize()
    assert float(bkg.min()) == -5.0 and int(status.item()) == -5
    assert maps(need, (None, None, vp(thr.data_ptr()))) == 0            # null outputs are honoured
    torch.cuda.synchronize()
    assert float(bkg.min()) == -5.0 and float(rms.min()) == -5.0 and float(thr.min()) > 50 and int(status.item()) == 0
    assert maps(need, (vp(bkg.data_ptr()), vp(rms.data_ptr()), None)) == 0
    torch.cuda.synchronize()
    st = bs.statement(fh, (bh, bw), nsigma=2.5)
    bs.check_mesh(mb.cpu().numpy(), mr.cpu().numpy(), ng.cpu().numpy(), st, 'raw pointers')
    bs.check_maps(bkg.cpu().numpy(), rms.cpu().numpy(), thr.cpu().numpy(), st, 'raw pointers')


def test_detect_sources_end_to_end():
    """512 x 512, 80 sources: detect_sources (which is given no background) against find_sources given the truth;
    and against find_sources given the STATEMENT's maps, from which it may differ only by the maps' bounds."""
    from subpixal_amd import detect
    fh, true_bkg, sigma = bc.e2e_scene()
    f = torch.from_numpy(fh).cuda()
    src = detect.detect_sources(f, nsigma=bc.E2E_NSIGMA, box=(64, 64), min_area=bc.E2E_MIN_AREA)
    assert src.background_model.background.shape == f.shape and src.segmentation.is_cuda
    ref = detect.find_sources(f, (true_bkg + bc.E2E_NSIGMA * sigma).astype(np.float32), background=true_bkg.astype(np.float32),
                              min_area=bc.E2E_MIN_AREA)
    xy = lambda s: np.stack([s.x, s.y], axis=1)[(s.flags & detect.FLAG_NOFLUX) == 0]
    share = bc.unmatched_share(xy(src), xy(ref))
    print('end to end: %d sources found, %d with the true background, unmatched share %.4f (statement: %.4f, cap %.2f)'
          % (len(src), len(ref), share, bc.E2E_STATEMENT_SHARE, bc.E2E_UNMATCHED_CAP))
    assert 70 <= len(ref) <= 90 and share <= bc.E2E_UNMATCHED_CAP
    # the statement's maps in place of the device's: no pixel of this scene lies within the threshold map's bound of
    # the threshold (tests/test_background_cpu.py), so the segmentations must be EQUAL, and with equal segments a
    # centroid sum(w x) / sum(w), w = v - bkg, moves by at most 2 npix bmap extent / flux for a background off by
    # bmap (first order in bmap npix / flux, which the scene keeps below 1e-3), plus the float32 rounding of the
    # statement's background map when it is handed over (inside bmap) and 1e-9 px for the measurements' own sums
    st = bs.statement(fh, (64, 64), nsigma=bc.E2E_NSIGMA)
    assert not np.any(np.abs(fh.astype(np.float64) - st['thr']) <= st['bthr'])
    bs.check_maps(src.background_model.background.cpu().numpy(), src.background_model.rms.cpu().numpy(),
                  src.background_model.threshold(bc.E2E_NSIGMA).cpu().numpy(), st, 'end to end')
    viast = detect.find_sources(f, st['thr'].astype(np.float32), background=st['bkg'].astype(np.float32),
                                min_area=bc.E2E_MIN_AREA)
    thr32 = st['thr'].astype(np.float32).astype(np.float64)
    assert not np.any(np.abs(fh.astype(np.float64) - thr32) <= st['bthr'])
    assert np.array_equal(viast.segmentation.cpu().numpy(), src.segmentation.cpu().numpy())
    bmap = float(st['bmap_bkg'].max())
    ext = np.maximum(src.bbox[:, 2] - src.bbox[:, 0], src.bbox[:, 3] - src.bbox[:, 1]) + 1.0
    assert np.all(src.npix * bmap <= 1e-3 * src.flux)
    bound = 2.0 * src.npix * bmap * ext / src.flux + 1e-9
    assert np.all(np.abs(src.x - viast.x) <= bound) and np.all(np.abs(src.y - viast.y) <= bound)
    # a second pass with the first one's sources excluded must not lower the share of matched sources
    src2 = detect.detect_sources(f, nsigma=bc.E2E_NSIGMA, box=(64, 64), min_area=bc.E2E_MIN_AREA, passes=2)
    share2 = bc.unmatched_share(xy(src2), xy(ref))
    print('two passes: %d sources, unmatched share %.4f' % (len(src2), share2))
    assert share2 <= share
