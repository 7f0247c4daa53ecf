"""The drizzle on the device: `resample.DeviceDrizzle` (spx_drizzle_f32 / _f64) on every case of
tests/drizzle_cases.py against the numpy scatter of tests/drizzle_statement.py; bit-identical to the kernel source run
on CPU threads; deterministic; dropping and adding frames against fresh objects; the C entries through raw
pointers."""
import numpy as np
import pytest

import drizzle_cases as dc
import drizzle_emu as de
import drizzle_statement as ds

pytestmark = pytest.mark.gpu
DTYPES = (np.float32, np.float64)


def make(c, dtype, **over):
    from subpixal_amd import resample
    frames, weights, masks, shapes, maps, active, K = de.arrays(c, dtype)
    a = dict(frames=frames, maps=maps, out_shape=c['out_shape'], weights=weights, masks=masks, pixfrac=c['pixfrac'],
             kernel=c['kernel'], fill=c['fill'])
    a.update(over)
    d = resample.DeviceDrizzle(**a)
    if active is not None:
        for k in range(K):
            if not active[k]:
                d._active[k] = False                       # (what fast_drop_image does, without the launch)
    return d


def outputs(d):
    return d.output_sci.cpu().numpy(), d.output_wht.cpu().numpy(), d.output_ctx.cpu().numpy()


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', sorted(dc.ALL))
def test_case_against_the_statement(name, dtype):
    c = dc.ALL[name]()
    got = outputs(make(c, dtype).execute())
    r = ds.check(*got, de.statement(name, c), what='%s %s' % (name, np.dtype(dtype).name))
    print(name, np.dtype(dtype).name, r)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', dc.BITWISE)
def test_bit_identical_to_the_kernel_on_cpu_threads(tmp_path_factory, name, dtype):
    c = dc.ALL[name]()
    assert same(outputs(make(c, dtype).execute()), de.run(de.load(tmp_path_factory), c, dtype))


@pytest.mark.parametrize('dtype', DTYPES)
def test_runs_are_identical_also_at_other_addresses(dtype):
    import torch
    c = dc.many_frames()
    d = make(c, dtype)
    first = outputs(d.execute())
    for _ in range(3):
        assert same(outputs(d.execute()), first)
    hold = [torch.empty(12345, device='cuda') for _ in range(3)]             # moves what is allocated next
    assert same(outputs(make(c, dtype).execute()), first)
    del hold


@pytest.mark.parametrize('dtype', DTYPES)
def test_drop_and_add_equal_fresh_objects(dtype):
    """sci and wht to the bit; ctx too once its bits are read by name (a dropped frame keeps its row, so its bit
    stays where it was and is zero)"""
    c = dc.mixed_shapes()
    frames, weights, masks, shapes, maps, active, K = de.arrays(c, dtype)

    def fresh(order):
        from subpixal_amd import resample
        return resample.DeviceDrizzle([frames[k] for k in order], maps[order], c['out_shape'], names=order,
                                      weights=[weights[k] for k in order]).execute()

    def by_name(d):
        bits = ds.ctx_bits(d.output_ctx.cpu().numpy(), len(d.table_names))
        return {n: bits[k] for k, n in enumerate(d.table_names)}

    d = fresh([0, 1, 2])
    d.fast_drop_image(1)
    f = fresh([0, 2])
    assert d.input_image_names == [0, 2] and same(outputs(d)[:2], outputs(f)[:2])
    bd, bf = by_name(d), by_name(f)
    assert not bd[1].any() and all(np.array_equal(bd[n], bf[n]) for n in (0, 2))
    d.fast_drop_image(0)
    d.fast_add_image(1)
    d.fast_add_image(0)
    f = fresh([2, 1, 0])
    assert d.input_image_names == [2, 1, 0] == d.table_names and same(outputs(d), outputs(f))
    # a new map for one frame: one row rewritten, the same as a fresh object with that map
    m = maps.copy()
    m[1, 2] += 3.25
    d.set_map(1, m[1])
    d.execute()
    from subpixal_amd import resample
    g = resample.DeviceDrizzle([frames[k] for k in (2, 1, 0)], m[[2, 1, 0]], c['out_shape'], names=[2, 1, 0],
                               weights=[weights[k] for k in (2, 1, 0)]).execute()
    assert same(outputs(d), outputs(g)) and not same(outputs(d), outputs(f))
    # a copy shares the frames and leaves the original alone
    q = d.copy()
    q.fast_drop_image(2)
    assert q.input_image_names == [1, 0] and d.input_image_names == [2, 1, 0]
    assert same(outputs(d.execute()), outputs(g))
    assert q._pool[2].data.data_ptr() == d._pool[2].data.data_ptr()


@pytest.mark.parametrize('dtype', DTYPES)
def test_c_entries_through_raw_pointers_write_exactly_their_outputs(dtype):
    """outputs one row too large, filled with a sentinel: the extra row stays, everything else is written"""
    import torch
    from subpixal_amd import _ffi, device
    device.init()
    lib = _ffi.load()
    c = dc.many_frames()
    frames, weights, masks, shapes, maps, active, K = de.arrays(c, dtype)
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    fd = [torch.from_numpy(f).cuda() for f in frames]
    wd = [torch.from_numpy(w).cuda() for w in weights]
    ft = np.array([t.data_ptr() for t in fd], np.uint64)
    wt = np.array([t.data_ptr() for t in wd], np.uint64)
    rows = np.zeros((K, _ffi.DRIZZLE_ROW_BYTES), np.uint8)
    NY, NX = c['out_shape']
    assert lib.spx_drizzle_rows(ft.ctypes.data, wt.ctypes.data, None, shapes.ctypes.data, maps.ctypes.data, None, K,
                                c['pixfrac'], 0, NY, NX, rows.ctypes.data) == 0
    rd = torch.from_numpy(rows).cuda()
    sci = torch.full((NY + 1, NX), -77.0, dtype=tdt, device='cuda')
    wht = torch.full((NY + 1, NX), -77.0, dtype=torch.float32, device='cuda')
    ctx = torch.full((2 * NY + 1, NX), -77, dtype=torch.int32, device='cuda')
    fn = lib.spx_drizzle_f64 if dtype == np.float64 else lib.spx_drizzle_f32
    assert fn(rd.data_ptr(), K, 0, c['fill'], NY, NX, sci.data_ptr(), wht.data_ptr(), ctx.data_ptr(),
              device.stream_ptr()) == 0
    torch.cuda.synchronize()
    s, w, x = sci.cpu().numpy(), wht.cpu().numpy(), ctx.cpu().numpy()
    assert np.all(s[NY] == -77) and np.all(w[NY] == -77) and np.all(x[2 * NY] == -77)
    got = (s[:NY], w[:NY], x[:2 * NY].reshape(2, NY, NX))
    ds.check(*got, de.statement('many_frames', c), what='raw')
    assert same(got, outputs(make(c, dtype).execute()))


def test_a_refused_map_is_a_value_error_and_config_changes_take_effect():
    c = dc.rot30()
    d = make(c, np.float32).execute()
    with pytest.raises(ValueError, match='8 x 8'):
        d.set_map(0, [0.1, 0, 0, 0, 0.1, 0])
    d.set_map(0, c['maps'][0])
    first = outputs(d.execute())
    d.set_config_parameters(pixfrac=0.5, kernel='turbo', fill=-3.0)
    got = outputs(d.execute())
    c2 = dict(c, pixfrac=0.5, kernel='turbo', fill=-3.0)
    ds.check(*got, ds.statement(c2['frames'], c2['maps'], c2['out_shape'], weights=c2['weights'], pixfrac=0.5,
                                kernel='turbo', fill=-3.0), what='turbo after square')
    assert not same(got, first)
