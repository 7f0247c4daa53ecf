"""Scenes and the case runner shared by tests/test_background_cpu.py (CPU harness) and
tests/test_gpu_background.py (device): the same cases are checked against tests/background_statement.py on both.
A `run` callable takes (frame, box, filter_size, mask, exclude, sigma, max_iters, min_good_fraction, nsigma) and
returns a dict with mesh_bkg, mesh_rms, ngood (unfiltered mesh), filt_bkg, filt_rms, bkg, rms, thr and,
where the backend can see them, trace = float64 [ncy, ncx, 5] (lo, hi, med, mean, std).  Not a test module."""
import numpy as np
from scipy import ndimage

import background_statement as bs

DEFAULTS = dict(filter_size=3, mask=None, exclude=None, sigma=3.0, max_iters=10, min_good_fraction=0.5, nsigma=2.5)


def sky(shape, seed, dtype, noise=2.0):
    """Gaussian noise on a tilted plane plus a quadratic term"""
    ny, nx = shape
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:ny, 0:nx].astype(np.float64)
    f = 100.0 + 0.02 * xx + 0.03 * yy + 1e-4 * (xx - 0.4 * nx) ** 2 + rng.normal(0.0, noise, shape)
    return f.astype(dtype)


def with_blob(f, cy, cx, amp=300.0, sig=4.5):
    yy, xx = np.mgrid[0:f.shape[0], 0:f.shape[1]].astype(np.float64)
    return (f + amp * np.exp(-0.5 * ((yy - cy) ** 2 + (xx - cx) ** 2) / sig ** 2)).astype(f.dtype)


def blob_scene(dtype):
    """a bright Gaussian blob (above 10 sigma of the noise on a third of cell (1, 1) of a 32 x 32 mesh)"""
    return with_blob(sky((96, 96), 5, dtype), 48.0, 47.0, amp=400.0, sig=4.5)


def check_blob_cell(st, got):
    """the clip of the blob's cell takes more than one round (all 10: its wings keep feeding the edge), ends on a
    range that is still skewed and so takes the median"""
    c = st['mesh']['cells'][(1, 1)]
    assert c['rounds'] > 1 and c['branch'] == 'med' and c['hi'] < 0.7 * 32 * 32
    assert got['mesh_bkg'][1, 1] == c['med']
    assert c['history'][1] != c['history'][0] and c['history'][-1] != c['history'][1]


# (name, shape, box, dtype): the mesh geometries
GEOMETRY = [
    ('partial cells', (150, 203), (32, 48), np.float32),
    ('partial cells', (150, 203), (32, 48), np.float64),
    ('8x8 boxes', (37, 29), (8, 8), np.float32),
    ('8x8 boxes', (37, 29), (8, 8), np.float64),
    ('one cell', (20, 20), (64, 64), np.float32),
    ('one cell', (20, 20), (64, 64), np.float64),
    ('one knot in y', (64, 300), (64, 64), np.float32),
    ('one knot in y', (64, 300), (64, 64), np.float64),
    ('two knots', (100, 100), (64, 64), np.float32),
    ('two knots', (100, 100), (64, 64), np.float64),
    ('largest cells', (130, 257), (128, 128), np.float32),
    ('largest cells', (130, 70), (128, 64), np.float64),
]


def check_case(run, frame, box, what, expect_trace=False, **kw):
    """statement and backend on one case; every comparison of the issue.  Returns (statement, got)."""
    a = dict(DEFAULTS)
    a.update(kw)
    st = bs.statement(frame, box, a['filter_size'], a['mask'], a['exclude'], a['sigma'], a['max_iters'],
                      a['min_good_fraction'], nsigma=a['nsigma'])
    got = run(frame, box, **a)
    bs.check_mesh(got['mesh_bkg'], got['mesh_rms'], got['ngood'], st, what)
    if got.get('trace') is not None:
        tr = got['trace']
        bs.check_cells({k: (int(tr[k][0]), int(tr[k][1]), tr[k][2], tr[k][3], tr[k][4]) for k in st['mesh']['cells']},
                       st, what)
    else:
        assert not expect_trace
    bs.check_maps(got['bkg'], got['rms'], got['thr'], st, what, filt=(got['filt_bkg'], got['filt_rms']))
    # clamping: every pixel at or outside the first / last knot of an axis repeats the knot's row / column
    for m in (got['bkg'], got['rms']):
        c0y, c0x = (box[0] - 1) // 2, (box[1] - 1) // 2
        ncy, ncx = st['filt_bkg'].shape
        ly, lx = int(np.ceil((ncy - 1) * box[0] + (box[0] - 1) / 2.0)), int(np.ceil((ncx - 1) * box[1] + (box[1] - 1) / 2.0))
        for r in range(min(c0y, m.shape[0] - 1)):
            assert np.array_equal(m[r], m[min(c0y, m.shape[0] - 1)]), (what, 'rows above the first knot')
        for r in range(ly + 1, m.shape[0]):
            assert np.array_equal(m[r], m[ly]), (what, 'rows below the last knot')
        assert np.array_equal(m[:, 0], m[:, min(c0x, m.shape[1] - 1)]), (what, 'columns left of the first knot')
        if lx < m.shape[1] - 1:
            assert np.array_equal(m[:, -1], m[:, lx]), (what, 'columns right of the last knot')
    return st, got


def undershoot_scene(dtype):
    """constant sky but for one noisy cell: the rms spline through (0 .. 0 s 0 .. 0) dips below zero beside it"""
    f = np.full((64, 72), 10.0, dtype)
    rng = np.random.default_rng(41)
    f[24:32, 32:40] += rng.normal(0.0, 5.0, (8, 8)).astype(dtype)
    return f


# ---------------------------------------------------------------------------------------------------------------
# end to end: ~80 Gaussian sources on a sloped background with noise, 512 x 512
# ---------------------------------------------------------------------------------------------------------------
E2E_NSIGMA, E2E_MIN_AREA, E2E_NOISE = 3.0, 5, 2.0
E2E_UNMATCHED_CAP = 0.05        # see e2e_scene
E2E_STATEMENT_SHARE = 0.0       # what the statement's maps give on this scene (test_background_cpu.py asserts it)


def e2e_scene(seed=77):
    """(frame float32, true background float64, sigma).  The cap on unmatched sources: every source peaks at 15
    sigma or more, so a source can only come or go, split or merge where the two thresholds (true and estimated,
    a few per cent of sigma apart) cut a blend or a noise peak differently: rare events, allowed for 5 % of the
    sources (4 of 80).  The statement's own share on this scene is E2E_STATEMENT_SHARE."""
    ny = nx = 512
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:ny, 0:nx].astype(np.float64)
    bkg = 100.0 + 0.03 * xx - 0.02 * yy
    f = bkg + rng.normal(0.0, E2E_NOISE, (ny, nx))
    for _ in range(80):
        cy, cx = rng.uniform(8, ny - 8), rng.uniform(8, nx - 8)
        s = rng.uniform(1.2, 2.2)
        f += rng.uniform(30.0, 400.0) * np.exp(-0.5 * ((yy - cy) ** 2 + (xx - cx) ** 2) / s ** 2)
    return f.astype(np.float32), bkg, E2E_NOISE


def host_sources(frame, thr, bkg, min_area=E2E_MIN_AREA):
    """(x, y) of the 8-connected components of frame > thr with at least min_area pixels, flux-weighted"""
    lab, n = ndimage.label(np.asarray(frame, np.float64) > thr, structure=np.ones((3, 3), int))
    if n == 0:
        return np.zeros((0, 2))
    area = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    ids = np.flatnonzero(area >= min_area) + 1
    com = ndimage.center_of_mass(np.asarray(frame, np.float64) - bkg, lab, ids)
    return np.array([(c[1], c[0]) for c in com]).reshape(-1, 2)


def unmatched_share(a, b, radius=1.0):
    """share of the sources of either list without a partner within `radius` px in the other"""
    if len(a) == 0 and len(b) == 0:
        return 0.0
    if len(a) == 0 or len(b) == 0:
        return 1.0
    d = np.hypot(a[:, None, 0] - b[None, :, 0], a[:, None, 1] - b[None, :, 1])
    return float(((d.min(axis=1) > radius).sum() + (d.min(axis=0) > radius).sum()) / (len(a) + len(b)))
