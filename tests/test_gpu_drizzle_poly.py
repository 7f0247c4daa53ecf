"""The drizzle through polynomial maps on the device: `resample.DeviceDrizzle` with `PolyMap` entries
(spx_drizzle_poly_f32 / _f64) on every case of tests/drizzle_poly_cases.py against the numpy scatter of
tests/drizzle_poly_statement.py; bit-identical to the kernel source run on CPU threads; deterministic; dropping and
adding frames against fresh objects; the C entries through raw pointers; a refused map changes nothing."""
import numpy as np
import pytest

import drizzle_poly_cases as pc
import drizzle_poly_emu as pe
import drizzle_poly_statement as dps

pytestmark = pytest.mark.gpu
DTYPES = (np.float32, np.float64)


def make(c, dtype, **over):
    from subpixal_amd import resample
    frames, weights, masks, shapes, active, K = pe.arrays(c, dtype)
    a = dict(frames=frames, maps=c['maps'], out_shape=c['out_shape'], weights=weights, masks=masks,
             pixfrac=c['pixfrac'], kernel=c['kernel'], fill=c['fill'])
    a.update(over)
    d = resample.DeviceDrizzle(**a)
    if active is not None:
        for k in range(K):
            if not active[k]:
                d.fast_drop_image(k)
    return d


def outputs(d):
    return d.output_sci.cpu().numpy(), d.output_wht.cpu().numpy(), d.output_ctx.cpu().numpy()


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', sorted(pc.ALL))
def test_case_against_the_statement(name, dtype):
    c = pc.ALL[name]()
    d = make(c, dtype).execute()
    assert d._rows_poly
    r = dps.check(*outputs(d), pe.statement(name, c), what='%s %s' % (name, np.dtype(dtype).name))
    print(name, np.dtype(dtype).name, r)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', pc.BITWISE)
def test_bit_identical_to_the_kernel_on_cpu_threads(tmp_path_factory, name, dtype):
    c = pc.ALL[name]()
    assert same(outputs(make(c, dtype).execute()), pe.run(pe.load(tmp_path_factory), c, dtype))


@pytest.mark.parametrize('dtype', DTYPES)
def test_runs_are_identical_also_at_other_addresses(dtype):
    import torch
    c = pc.many_frames()
    d = make(c, dtype)
    first = outputs(d.execute())
    for _ in range(3):
        assert same(outputs(d.execute()), first)
    hold = [torch.empty(12345, device='cuda') for _ in range(3)]             # moves what is allocated next
    assert same(outputs(make(c, dtype).execute()), first)
    del hold


@pytest.mark.parametrize('dtype', DTYPES)
def test_drop_and_add_equal_fresh_objects(dtype):
    """a mixed table ([6] and PolyMap entries): sci and wht to the bit, ctx once its bits are read by name"""
    c = pc.mixed()
    frames, weights, masks, shapes, active, K = pe.arrays(c, dtype)
    maps = c['maps']

    def fresh(order, maps=maps):
        from subpixal_amd import resample
        return resample.DeviceDrizzle([frames[k] for k in order], [maps[k] for k in order], c['out_shape'], names=order,
                                      weights=[weights[k] for k in order]).execute()

    def by_name(d):
        bits = dps.ctx_bits(d.output_ctx.cpu().numpy(), len(d.table_names))
        return {n: bits[k] for k, n in enumerate(d.table_names)}

    d = fresh([0, 1, 2])
    d.fast_drop_image(1)
    f = fresh([0, 2])                                      # ([6] and a PolyMap: still the polynomial rows)
    assert d.input_image_names == [0, 2] and same(outputs(d)[:2], outputs(f)[:2])
    bd, bf = by_name(d), by_name(f)
    assert not bd[1].any() and all(np.array_equal(bd[n], bf[n]) for n in (0, 2))
    d.fast_drop_image(0)
    d.fast_add_image(1)
    d.fast_add_image(0)
    f = fresh([2, 1, 0])
    assert d.input_image_names == [2, 1, 0] == d.table_names and same(outputs(d), outputs(f))
    # a new map for one frame: one row rewritten, the same as a fresh object with that map
    m = list(maps)
    m[1] = pc.distorted(40, 48, deg=10.0, scale=0.6, tx=33.25, ty=20.0, k=4.0e-5)
    d.set_map(1, m[1])
    assert d.map(1) is m[1]
    d.execute()
    g = fresh([2, 1, 0], maps=m)
    assert same(outputs(d), outputs(g)) and not same(outputs(d), outputs(f))
    # a copy shares the frames and leaves the original alone
    q = d.copy()
    q.fast_drop_image(2)
    assert q.input_image_names == [1, 0] and d.input_image_names == [2, 1, 0]
    assert same(outputs(d.execute()), outputs(g))
    assert q._pool[2].data.data_ptr() == d._pool[2].data.data_ptr()
    # the last PolyMap leaves: the table is packed again for the affine kernel, bit for bit a fresh affine object
    a1, a2 = m[1].affine(), m[2].affine()
    d.set_map(1, a1)
    d.set_map(2, a2)
    d.execute()
    assert not d._rows_poly
    assert same(outputs(d), outputs(fresh([2, 1, 0], maps=[m[0], a1, a2])))


@pytest.mark.parametrize('dtype', DTYPES)
def test_c_entries_through_raw_pointers_write_exactly_their_outputs(dtype):
    """outputs one row too large, filled with a sentinel: the extra row stays, everything else is written"""
    import torch
    from subpixal_amd import _ffi, device
    device.init()
    lib = _ffi.load()
    c = pc.many_frames()
    frames, weights, masks, shapes, active, K = pe.arrays(c, dtype)
    coef, degree, center = pe.map_tables(c['maps'])
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    fd = [torch.from_numpy(f).cuda() for f in frames]
    wd = [torch.from_numpy(w).cuda() for w in weights]
    ft = np.array([t.data_ptr() for t in fd], np.uint64)
    wt = np.array([t.data_ptr() for t in wd], np.uint64)
    rows = np.zeros((K, _ffi.DRIZZLE_POLY_ROW_BYTES), np.uint8)
    NY, NX = c['out_shape']
    assert lib.spx_drizzle_poly_rows(ft.ctypes.data, wt.ctypes.data, None, shapes.ctypes.data, coef.ctypes.data,
                                     degree.ctypes.data, center.ctypes.data, None, K, c['pixfrac'], 0, NY, NX,
                                     rows.ctypes.data) == 0
    rd = torch.from_numpy(rows).cuda()
    sci = torch.full((NY + 1, NX), -77.0, dtype=tdt, device='cuda')
    wht = torch.full((NY + 1, NX), -77.0, dtype=torch.float32, device='cuda')
    ctx = torch.full((2 * NY + 1, NX), -77, dtype=torch.int32, device='cuda')
    fn = lib.spx_drizzle_poly_f64 if dtype == np.float64 else lib.spx_drizzle_poly_f32
    assert fn(rd.data_ptr(), K, 0, c['fill'], NY, NX, sci.data_ptr(), wht.data_ptr(), ctx.data_ptr(),
              device.stream_ptr()) == 0
    torch.cuda.synchronize()
    s, w, x = sci.cpu().numpy(), wht.cpu().numpy(), ctx.cpu().numpy()
    assert np.all(s[NY] == -77) and np.all(w[NY] == -77) and np.all(x[2 * NY] == -77)
    got = (s[:NY], w[:NY], x[:2 * NY].reshape(2, NY, NX))
    dps.check(*got, pe.statement('many_frames', c), what='raw')
    assert same(got, outputs(make(c, dtype).execute()))


def test_a_refused_polymap_changes_nothing_and_config_changes_take_effect():
    c = pc.radial3()
    d = make(c, np.float32).execute()
    first = outputs(d)
    rows = d._rows_host.copy()
    with pytest.raises(ValueError, match='8 x 8'):
        d.set_map(0, pc.too_small()['maps'][0])
    with pytest.raises(ValueError, match='singular'):
        d.set_map(0, pc.folded()['maps'][0])
    assert d.map(0) is c['maps'][0] and np.array_equal(d._rows_host, rows)
    assert np.array_equal(d._rows_dev.cpu().numpy(), rows) and same(outputs(d.execute()), first)
    d.set_config_parameters(pixfrac=0.8, kernel='turbo')
    c2 = pc.radial3_turbo()
    dps.check(*outputs(d.execute()), pe.statement('radial3_turbo', c2), what='turbo after square')
    # an affine drizzle that receives its first PolyMap, refused: it stays an affine drizzle, bit for bit
    from subpixal_amd import resample
    frames, weights, masks, shapes, active, K = pe.arrays(c, np.float32)
    a = resample.DeviceDrizzle(frames, [c['maps'][0].affine()], c['out_shape'], weights=weights).execute()
    before = outputs(a)
    with pytest.raises(ValueError, match='8 x 8'):
        a.set_map(0, pc.too_small()['maps'][0])
    assert not a._rows_poly and same(outputs(a.execute()), before)
