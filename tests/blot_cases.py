"""Cases for the half-pixel dithered blots (spx_aux_kernels.h: everett5, blot_sample, blot_resample,
blot_poly_eval and the three kernels around them) at the edges of small sources, written once and run by
tests/test_blot_edges_cpu.py (CPU threads, tests/emu.py) and tests/test_gpu_blot_edges.py (the MI355X).

The expected values come from the oracle's float64 Lagrange statement only (oracle/subpixal_oracle.py:
_lagrange6, _continued; `expected` below is _blot4's loop, which also keeps the continued 6x6 patch the bound is
taken from, and `check_restates_oracle` holds it to blot_affine4 / blot_map4 bit for bit).  Every map
coefficient and target coordinate is a dyadic rational, so the source position (xs, ys) is exact in double
with or without FMA contraction: kernel and oracle agree on inside / outside and on the cell (ix, iy) for
every pixel, and nothing has to be excluded from a comparison.

A backend is an object with
    affine(src [N, sny, snx], aff [N, 6], (ny, nx), gain) -> float32 [N, 4, ny, nx]
    poly(src, coef [N, 2, 21], degree, (ny, nx), gain)    -> float32 [N, 4, ny, nx]
    packed(src, src_offs, src_shapes, maps, degree, dst_offs, dst_shapes, out, gain) -> out after the launch,
        `out` a float32 or float64 array the caller filled (it selects the float32 or the float64 instance)
"""
import functools

import numpy as np

from oracle import subpixal_oracle as orc

EPS = 2.0 ** -24                 # half an ulp of a float32 in [1, 2)
DITHERS = ((0.0, 0.0), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5))
SHAPES = ((6, 6), (6, 9), (9, 6), (7, 10), (12, 12), (13, 11))        # (sny, snx)
POLY_TERMS = 21
SENTINEL = -7.0
KERNELS = ('affine', 'poly1', 'packed')

# The per-pixel bound |got - exp| <= C * 2^-24 * max|continued 6x6 patch|.  Measured over all group-3 cases
# against the float64 oracle (profiles/r06/blot_edges.txt): 2.523 on CPU threads for each of the three kernels;
# C is twice the larger measured value.  (The array-wide 5e-6 * max|exp| of the older tests is about 84 of
# these units.)
C = 5.05

BAND = ('0', '1', 'mid', 'n-4', 'n-3', 'n-2', 'n-1')
FRACS = (0.0, 0.125, 0.5, 0.875)


def band_class(i, n):
    """Index into BAND of cell i of an n-sample axis (for n = 6 there is no 'mid')."""
    if i < 2:
        return i
    return 3 + i - (n - 4) if i >= n - 4 else 2


def band_classes(n):
    return sorted({band_class(i, n) for i in range(n)})


# ---------------------------------------------------------------------------------------------------------------
# expected values
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _weights(s):
    return orc._lagrange6(s)


def _extended(tile):
    """orc._continued at every index a 6x6 patch can touch: [-2, n + 2] per axis"""
    sny, snx = tile.shape
    return np.array([[orc._continued(tile, j, i) for i in range(-2, snx + 3)] for j in range(-2, sny + 3)])


class Expected:
    """One source through one map: float64 [4, ny, nx] arrays.  `exp` the blots, `pmax` max|continued 6x6
    patch| (0 outside), `ix`, `iy` the cell (-1 outside), `fx`, `fy` the fractional position."""

    def __init__(self, tile, mapping, ny, nx):
        tile = np.asarray(tile, dtype=np.float64)
        sny, snx = tile.shape
        ext = _extended(tile)
        self.exp = np.zeros((4, ny, nx))
        self.pmax = np.zeros((4, ny, nx))
        self.ix = np.full((4, ny, nx), -1)
        self.iy = np.full((4, ny, nx), -1)
        self.fx = np.zeros((4, ny, nx))
        self.fy = np.zeros((4, ny, nx))
        for q, (ox, oy) in enumerate(DITHERS):
            for y in range(ny):
                for x in range(nx):
                    xs, ys = mapping(x + ox, y + oy)
                    if not (0.0 <= xs <= snx - 1 and 0.0 <= ys <= sny - 1):
                        continue
                    i, j = int(np.floor(xs)), int(np.floor(ys))
                    patch = np.ascontiguousarray(ext[j:j + 6, i:i + 6])     # samples (j-2..j+3, i-2..i+3)
                    self.exp[q, y, x] = _weights(ys - j) @ patch @ _weights(xs - i)
                    self.pmax[q, y, x] = np.nanmax(np.abs(patch))
                    self.ix[q, y, x], self.iy[q, y, x] = i, j
                    self.fx[q, y, x], self.fy[q, y, x] = xs - i, ys - j


def affine_map(a):
    a = [float(v) for v in a]
    return lambda xt, yt: (a[0] * xt + a[1] * yt + a[2], a[3] * xt + a[4] * yt + a[5])


class Case:
    """A batch of sources of one shape through per-source maps onto one target shape, with the oracle's
    answer.  `aff` [N, 6] for affine maps; `coef` [N, 2, 21] and `degree` for polynomial ones (affine cases
    carry their degree-1 coefficients)."""

    def __init__(self, name, src, shape, aff=None, coef=None, degree=1, mappings=None, gain=None):
        self.name = name
        self.src = np.ascontiguousarray(src, dtype=np.float32)
        self.shape = ny, nx = int(shape[0]), int(shape[1])
        self.aff = None if aff is None else np.ascontiguousarray(aff, dtype=np.float64)
        self.coef = affine_to_coef(self.aff, self.shape) if coef is None else np.ascontiguousarray(coef)
        self.degree = degree
        self.gain = None if gain is None else np.ascontiguousarray(gain, dtype=np.float32)
        self.mappings = [affine_map(a) for a in self.aff] if mappings is None else list(mappings)
        per = [Expected(t, m, ny, nx) for t, m in zip(self.src, self.mappings)]
        for f in ('exp', 'pmax', 'ix', 'iy', 'fx', 'fy'):
            setattr(self, f, np.stack([getattr(e, f) for e in per]))
        if self.gain is not None:
            g = self.gain.astype(np.float64)[:, None, None, None]
            self.exp, self.pmax = self.exp * g, self.pmax * np.abs(g)
        for a in (self.src, self.aff, self.coef, self.gain, self.exp, self.pmax, self.ix, self.iy, self.fx, self.fy):
            if a is not None:
                a.setflags(write=False)                         # shared between tests: leave it unchanged
        self.inside = self.ix >= 0

    @property
    def pixels(self):
        return self.exp.size


def affine_to_coef(aff, shape):
    """[N, 6] affines as degree-1 coefficients of the polynomial kernel (u = x - (nx-1)/2, v = y - (ny-1)/2)"""
    a = np.asarray(aff, dtype=np.float64)
    xc, yc = 0.5 * (shape[1] - 1), 0.5 * (shape[0] - 1)
    c = np.zeros((len(a), 2, POLY_TERMS))
    c[:, 0, 0] = a[:, 2] + a[:, 0] * xc + a[:, 1] * yc
    c[:, 0, 1], c[:, 0, 2] = a[:, 0], a[:, 1]
    c[:, 1, 0] = a[:, 5] + a[:, 3] * xc + a[:, 4] * yc
    c[:, 1, 1], c[:, 1, 2] = a[:, 3], a[:, 4]
    return c


def slot(i, j):
    """the kernel's slot of u^i v^j: k = d (d + 1) / 2 + (d - i), d = i + j"""
    d = i + j
    return d * (d + 1) // 2 + (d - i)


def check_restates_oracle(case):
    """`Expected` is the oracle's own loop: bit for bit what blot_map4 returns"""
    want = orc.blot_map4(case.src, case.mappings, case.shape[0], case.shape[1], case.gain)
    assert np.array_equal(case.exp, want, equal_nan=True), case.name


# ---------------------------------------------------------------------------------------------------------------
# running a case through a kernel
# ---------------------------------------------------------------------------------------------------------------
def pack_layout(shapes, gap):
    """offsets (in pixels) of items of `shapes` with `gap` unused pixels before, between and after them"""
    sizes = np.array([int(h) * int(w) for h, w in shapes], dtype=np.int64)
    offs = gap + np.concatenate([[0], np.cumsum(sizes + gap)[:-1]]).astype(np.int64)
    return offs, int(offs[-1] + sizes[-1] + gap)


def run_packed(backend, tiles, maps, degree, dst_shapes, gain=None, dtype=np.float32, gap=3):
    """One launch of the packed kernel over 2-D `tiles` of any shapes; the source is laid out with NaN between
    the tiles (a read outside a tile shows), the destination with SENTINEL before, between and after the items,
    which must survive.  Returns the items' [4, ny, nx] blots."""
    src_shapes = np.array([t.shape for t in tiles], dtype=np.int32)
    dst_shapes = np.array(dst_shapes, dtype=np.int32)
    soffs, stotal = pack_layout(src_shapes, 2)
    doffs, dtotal = pack_layout(dst_shapes, gap)
    src = np.full(stotal, np.nan, dtype=np.float32)
    used = np.zeros(4 * dtotal, dtype=bool)
    for t, o in zip(tiles, soffs):
        src[o:o + t.size] = np.asarray(t, dtype=np.float32).ravel()
    for (h, w), o in zip(dst_shapes, doffs):
        used[4 * o:4 * o + 4 * h * w] = True
    out = np.full(4 * dtotal, SENTINEL, dtype=dtype)
    got = backend.packed(src, soffs, src_shapes, np.ascontiguousarray(maps, dtype=np.float64), degree, doffs,
                         dst_shapes, out, gain)
    assert got.dtype == dtype and got.shape == (4 * dtotal,)
    assert np.count_nonzero(~used) >= 4 * gap * (len(tiles) + 1)
    assert np.all(got[~used] == SENTINEL), "the launch wrote outside its items"
    return [got[4 * o:4 * o + 4 * h * w].reshape(4, h, w) for (h, w), o in zip(dst_shapes, doffs)]


def run_cases(backend, kernel, cases):
    """the [N, 4, ny, nx] results of `cases` through 'affine', 'poly1' (the polynomial kernel at degree 1) or
    'packed' (all items of all cases, whatever their shapes, in ONE launch)"""
    if kernel == 'affine':
        return [backend.affine(c.src, c.aff, c.shape, c.gain) for c in cases]
    if kernel == 'poly1':
        return [backend.poly(c.src, c.coef, 1, c.shape, c.gain) for c in cases]
    assert kernel == 'packed'
    tiles = [t for c in cases for t in c.src]
    maps = np.concatenate([c.aff for c in cases])
    shapes = [c.shape for c in cases for _ in c.src]
    gain = None
    if any(c.gain is not None for c in cases):
        gain = np.concatenate([np.ones(len(c.src), np.float32) if c.gain is None else c.gain for c in cases])
    items = run_packed(backend, tiles, maps, 0, shapes, gain)
    out, k = [], 0
    for c in cases:
        out.append(np.stack(items[k:k + len(c.src)]))
        k += len(c.src)
    return out


def ratio(got, case):
    """|got - exp| in units of 2^-24 max|patch|, per pixel (0 where the point is outside the source or the
    expected value is NaN)"""
    ok = case.inside & ~np.isnan(case.exp)
    r = np.zeros(case.exp.shape)
    r[ok] = np.abs(got.astype(np.float64)[ok] - case.exp[ok]) / (EPS * case.pmax[ok])
    return r


def check_bound(got, case, what=''):
    """same shape and type, the same pixels outside the source, every pixel within the bound; returns the
    worst ratio (printed before it is asserted)"""
    assert got.shape == case.exp.shape and got.dtype == np.float32
    assert np.array_equal(got == 0, case.exp == 0), (case.name, what)
    assert np.array_equal(np.isnan(got), np.isnan(case.exp)), (case.name, what)
    r = ratio(got, case)
    worst = float(r.max())
    print('%-8s %-28s max |got - exp| / (2^-24 max|patch|) = %.3f' % (what, case.name, worst))
    assert worst <= C, (case.name, what, worst, np.unravel_index(r.argmax(), r.shape))
    return worst


# ---------------------------------------------------------------------------------------------------------------
# group 1: integer translations
# ---------------------------------------------------------------------------------------------------------------
G1_OFFSETS = ((-2, -2), (0, 0), (3, -4), (-5, 1))        # (x0, y0): before the source, on it, past the far edge


@functools.lru_cache(maxsize=None)
def group1():
    """every source shape, identity scale, integer offsets, onto a target 4 px larger than the source: with
    (-2, -2) the target covers the whole source, its last row and column and all four corners, and a 2 px rim
    outside; (0, 0) ends 3 px past the far edges"""
    rng = np.random.default_rng(601)
    cases = []
    for sny, snx in SHAPES:
        src = rng.normal(size=(len(G1_OFFSETS), sny, snx)).astype(np.float32)
        aff = np.array([[1, 0, x0, 0, 1, y0] for x0, y0 in G1_OFFSETS], dtype=np.float64)
        cases.append(Case('shift %dx%d' % (sny, snx), src, (sny + 4, snx + 4), aff))
    return tuple(cases)


def shifted(case):
    """dither 00 of a group-1 case by slicing: the source moved by whole pixels, 0 outside"""
    n, sny, snx = case.src.shape
    ny, nx = case.shape
    out = np.zeros((n, ny, nx), dtype=np.float32)
    for b, (x0, y0) in enumerate(G1_OFFSETS):
        ys, xs = np.arange(ny) + y0, np.arange(nx) + x0
        vy, vx = (ys >= 0) & (ys <= sny - 1), (xs >= 0) & (xs <= snx - 1)
        out[b][np.ix_(vy, vx)] = case.src[b][np.ix_(ys[vy], xs[vx])]
    return out


def check_group1(backend, kernel):
    cases = group1()
    for case, got in zip(cases, run_cases(backend, kernel, cases)):
        n, sny, snx = case.src.shape
        want = shifted(case)
        # the case reaches the far edge itself (xs == snx-1, ys == sny-1) and all four corners
        on = case.ix[:, 0], case.iy[:, 0]
        for cx in (0, snx - 1):
            for cy in (0, sny - 1):
                assert np.any((on[0] == cx) & (on[1] == cy)), (case.name, cx, cy)
        assert np.any(~case.inside[:, 0])
        assert np.array_equal(got[:, 0], want), (case.name, kernel)          # bit for bit, 0 outside
        check_bound(got, case, kernel)                                       # dithers 10, 01, 11 (and 00)


# ---------------------------------------------------------------------------------------------------------------
# group 2: integer ramps
# ---------------------------------------------------------------------------------------------------------------
RAMPS = (('3x-2y+7', lambda x, y: 3.0 * x - 2.0 * y + 7.0), ('x', lambda x, y: x + 0.0 * y),
         ('y', lambda x, y: y + 0.0 * x))
G2_FRACS = ((0.0, 0.0), (0.125, 0.875), (0.625, 0.25), (0.875, 0.125), (0.0, 0.375))


def group2():
    """(name, src [N, sny, snx], aff [N, 6], shape, gain, want [N, 4, ny, nx]) for the three ramps on a 6x6 and
    a 7x10 source: unit scale, offsets -1 + f with f in eighths, targets 2 px larger than the source; `want`
    is ramp(xs, ys) inside, 0 outside -- exact in float32."""
    out = []
    for sny, snx in ((6, 6), (7, 10)):
        yy, xx = np.mgrid[0:sny, 0:snx].astype(np.float64)
        ny, nx = sny + 2, snx + 2
        aff = np.array([[1, 0, fx - 1, 0, 1, fy - 1] for fx, fy in G2_FRACS])
        n = len(aff)
        for name, ramp in RAMPS:
            for gain in (None, 2.0):
                if gain is not None and name != '3x-2y+7':
                    continue
                src = np.broadcast_to(ramp(xx, yy), (n, sny, snx)).astype(np.float32)
                want = np.zeros((n, 4, ny, nx))
                cells = np.zeros((sny, snx), dtype=int)
                for b in range(n):
                    for q, (ox, oy) in enumerate(DITHERS):
                        xs = np.arange(nx)[None, :] + ox + aff[b, 2] + 0.0 * np.arange(ny)[:, None]
                        ys = np.arange(ny)[:, None] + oy + aff[b, 5] + 0.0 * np.arange(nx)[None, :]
                        ins = (xs >= 0) & (xs <= snx - 1) & (ys >= 0) & (ys <= sny - 1)
                        want[b, q][ins] = ramp(xs[ins], ys[ins]) * (gain or 1.0)
                        np.add.at(cells, (np.floor(ys[ins]).astype(int), np.floor(xs[ins]).astype(int)), 1)
                assert cells.min() > 0, "a cell of the source gets no sample"
                assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
                g = None if gain is None else np.full(n, gain, np.float32)
                out.append(('%s %dx%d gain %s' % (name, sny, snx, gain), src, aff, (ny, nx), g,
                            want.astype(np.float32)))
    return out


def check_group2(backend, kernel):
    for name, src, aff, shape, gain, want in group2():
        if kernel == 'affine':
            got = backend.affine(src, aff, shape, gain)
        elif kernel == 'poly1':
            got = backend.poly(src, affine_to_coef(aff, shape), 1, shape, gain)
        else:
            got = np.stack(run_packed(backend, list(src), aff, 0, [shape] * len(src), gain))
        bad = np.argwhere(got != want)
        assert bad.size == 0, (name, kernel, len(bad), bad[:8].tolist())


# ---------------------------------------------------------------------------------------------------------------
# group 3: random sources at every band position
# ---------------------------------------------------------------------------------------------------------------
G3_SHAPES = ((6, 6), (7, 10), (12, 12))


@functools.lru_cache(maxsize=None)
def group3():
    """normal fields of 6x6, 7x10 and 12x12 through
      unit scale, offsets -1 + f, f in {0, 1/8, 7/8}^2 (the dithers add 1/2), targets 2 px larger than the source;
      scale 1/2 with the shear a1 = 1/8;
      scale 5/4 with the shear a3 = 1/8,
    and the check that every band class is reached (see check_group3_coverage)"""
    rng = np.random.default_rng(603)
    cases = []
    for sny, snx in G3_SHAPES:
        tile = rng.normal(size=(sny, snx)).astype(np.float32)
        unit = np.array([[1, 0, fx - 1, 0, 1, fy - 1] for fy in (0, 0.125, 0.875) for fx in (0, 0.125, 0.875)])
        half = np.array([[0.5, 0.125, -3.5, 0, 0.5, -0.5], [0.5, 0.125, -3.375, 0, 0.5, -0.375]])
        wide = np.array([[1.25, 0, -1, 0.125, 1.25, -1.5], [1.25, 0, -0.875, 0.125, 1.25, -1.125]])
        for name, aff, shape in (('unit', unit, (sny + 2, snx + 2)), ('half', half, (2 * sny + 2, 2 * snx + 4)),
                                 ('5/4', wide, (sny + 1, snx + 1))):
            src = np.broadcast_to(tile, (len(aff), sny, snx))
            cases.append(Case('%s %dx%d' % (name, sny, snx), src, shape, aff))
    return tuple(cases)


def check_group3_coverage():
    """per source: every (ix class, iy class) pair is reached, the four corners with them, and every class is
    reached at each fractional part in {0, 1/8, 1/2, 7/8} ('n-1' is the far edge itself: fraction 0 only)"""
    cases = group3()
    for shape in sorted({c.src.shape[1:] for c in cases}):
        sny, snx = shape
        pairs, fxs, fys = {}, {}, {}
        for c in (c for c in cases if c.src.shape[1:] == shape):
            m = c.inside
            for i, j, fx, fy in zip(c.ix[m], c.iy[m], c.fx[m], c.fy[m]):
                ci, cj = band_class(i, snx), band_class(j, sny)
                pairs[ci, cj] = pairs.get((ci, cj), 0) + 1
                fxs[ci, fx] = fxs.get((ci, fx), 0) + 1
                fys[cj, fy] = fys.get((cj, fy), 0) + 1
        for ci in band_classes(snx):
            for cj in band_classes(sny):
                assert pairs.get((ci, cj), 0) > 0, (shape, BAND[ci], BAND[cj])
        for n, seen in ((snx, fxs), (sny, fys)):
            for cl in band_classes(n):
                for f in ((0.0,) if BAND[cl] == 'n-1' else FRACS):
                    assert seen.get((cl, f), 0) > 0, (shape, BAND[cl], f)
    assert band_classes(6) == [0, 1, 3, 4, 5, 6] and band_classes(7) == list(range(7))


def check_group3(backend, kernel, shape):
    """the group-3 cases of one source shape (three target shapes: one launch of the packed kernel)"""
    cases = [c for c in group3() if c.src.shape[1:] == tuple(shape)]
    assert len(cases) == 3 and sum(c.pixels for c in cases) <= 20000
    worst = max(check_bound(got, case, kernel) for case, got in zip(cases, run_cases(backend, kernel, cases)))
    print('%-8s group 3, %dx%d: max ratio %.3f (C = %.2f)' % (kernel, shape[0], shape[1], worst, C))
    return worst


def measure_group3(backend):
    """{kernel: max |got - exp| / (2^-24 max|patch|) over all group-3 cases}, nothing asserted"""
    cases = group3()
    return {k: max(float(ratio(got, case).max()) for case, got in zip(cases, run_cases(backend, k, cases)))
            for k in KERNELS}


# ---------------------------------------------------------------------------------------------------------------
# group 4: every polynomial degree
# ---------------------------------------------------------------------------------------------------------------
G4_SHAPE = (9, 10)                                             # xc = 4.5, yc = 4


def poly_terms(degree):
    """{(i, j): (cx, cy)}: a dyadic map of total degree `degree` with EVERY monomial u^i v^j, i + j <= degree,
    present in both xs and ys, each with its own coefficient (so a wrong slot shows)"""
    t = {(0, 0): (5.5, 5.25), (1, 0): (1.25, -0.125), (0, 1): (0.125, 1.25)}
    for d in range(2, degree + 1):
        for j in range(d + 1):
            i = d - j
            t[i, j] = ((-1) ** j * (1 + j) * 2.0 ** -(2 * d + 3), (-1) ** i * (1 + i) * 2.0 ** -(2 * d + 3))
    return t


def poly_coef(terms, fill=0.0):
    c = np.full((2, POLY_TERMS), fill)
    for (i, j), (cx, cy) in terms.items():
        c[0, slot(i, j)], c[1, slot(i, j)] = cx, cy
    return c


def poly_map(terms, shape):
    xc, yc = 0.5 * (shape[1] - 1), 0.5 * (shape[0] - 1)

    def mapping(xt, yt):
        u, v = xt - xc, yt - yc
        return (sum(cx * u ** i * v ** j for (i, j), (cx, _) in terms.items()),
                sum(cy * u ** i * v ** j for (i, j), (_, cy) in terms.items()))
    return mapping


@functools.lru_cache(maxsize=None)
def group4():
    """{degree: Case}: one 12x12 normal field through the degree-d map onto a 9x10 target"""
    rng = np.random.default_rng(604)
    tile = rng.normal(size=(1, 12, 12)).astype(np.float32)
    cases = {}
    for degree in range(1, 6):
        terms = poly_terms(degree)
        assert len(terms) == (degree + 1) * (degree + 2) // 2
        assert sorted(slot(i, j) for i, j in terms) == list(range(len(terms)))
        case = Case('degree %d' % degree, tile, G4_SHAPE, coef=poly_coef(terms)[None], degree=degree,
                    mappings=[poly_map(terms, G4_SHAPE)])
        # the map keeps most of the target on the source and some of it off, and reaches the edge band
        assert 0.5 * case.pixels < case.inside.sum() < case.pixels, case.name
        assert np.any(case.inside & ((case.ix < 2) | (case.ix > 8) | (case.iy < 2) | (case.iy > 8)))
        cases[degree] = case
    return cases


def check_group4(backend, degree):
    case = group4()[degree]
    check_restates_oracle(case)
    got = backend.poly(case.src, case.coef, degree, case.shape, None)
    check_bound(got, case, 'poly%d' % degree)
    # the slots above `degree` are not read
    nan_above = poly_coef(poly_terms(degree), fill=np.nan)[None]
    assert np.isnan(nan_above).sum() == 2 * (POLY_TERMS - (degree + 1) * (degree + 2) // 2)
    assert np.array_equal(backend.poly(case.src, nan_above, degree, case.shape, None), got)
    # ... nor by the packed kernel, which is the fixed-shape one bit for bit
    items = run_packed(backend, list(case.src), nan_above, degree, [case.shape])
    assert np.array_equal(items[0], got[0])
    if degree == 1:
        t = poly_terms(1)
        xc, yc = 0.5 * (case.shape[1] - 1), 0.5 * (case.shape[0] - 1)
        aff = np.array([[t[1, 0][k], t[0, 1][k], t[0, 0][k] - t[1, 0][k] * xc - t[0, 1][k] * yc] for k in (0, 1)])
        assert np.array_equal(backend.affine(case.src, aff.reshape(1, 6), case.shape, None), got)


# ---------------------------------------------------------------------------------------------------------------
# group 5: the packed kernel
# ---------------------------------------------------------------------------------------------------------------
G5_SRC = ((6, 6), (5, 9), (9, 5), (7, 10), (12, 12), (1, 1), (6, 6))
G5_DST = ((1, 1), (4, 7), (7, 4), (9, 12), (11, 13), (3, 3), (8, 8))


def check_group5(backend, degree):
    """a mix of source and target shapes in one launch, affine (degree 0) or cubic (degree 3), with and without
    gain: sources with a side below 6 px give zeros, every other item is the fixed-shape kernel's bit for bit, the
    float64 instance is the float32 one widened, nothing is written between the items"""
    rng = np.random.default_rng(605)
    tiles = [rng.normal(size=s).astype(np.float32) for s in G5_SRC]
    n = len(tiles)
    if degree == 0:
        maps = np.array([[1, 0, 2.125, 0, 1, 3.5], [1, 0, 0, 0, 1, 0], [1, 0, 0, 0, 1, 0],
                         [1, 0.125, -1.625, 0, 0.75, -0.5], [1.25, 0, -1, 0.125, 1.25, -1.5],
                         [1, 0, 0, 0, 1, 0], [1, 0, -0.875, 0, 1, -1.125]])
    else:
        maps = np.zeros((n, 2, POLY_TERMS))
        for k, ((sny, snx), (ny, nx)) in enumerate(zip(G5_SRC, G5_DST)):
            t = poly_terms(3)
            t[0, 0] = (0.5 * (snx - 1) + 0.125, 0.5 * (sny - 1) - 0.25)
            t[1, 0], t[0, 1] = (0.75, -0.125), (0.125, 0.75)
            maps[k] = poly_coef(t)
    seen = 0
    for gain in (None, rng.uniform(0.5, 2.0, n).astype(np.float32)):
        got = run_packed(backend, tiles, maps, degree, G5_DST, gain)
        wide = run_packed(backend, tiles, maps, degree, G5_DST, gain, dtype=np.float64, gap=5)
        for k, (tile, shape) in enumerate(zip(tiles, G5_DST)):
            assert got[k].dtype == np.float32 and wide[k].dtype == np.float64
            assert np.array_equal(wide[k], got[k].astype(np.float64)), (k, degree)
            if min(tile.shape) < 6:
                assert not got[k].any(), (k, degree)
                continue
            g = None if gain is None else gain[k:k + 1]
            if degree == 0:
                alone = backend.affine(tile[None], maps[k:k + 1], shape, g)
            else:
                alone = backend.poly(tile[None], maps[k:k + 1], degree, shape, g)
            assert np.array_equal(got[k], alone[0]), (k, degree)
            assert got[k].any(), (k, degree)
            seen += 1
    assert seen == 2 * sum(min(s) >= 6 for s in G5_SRC)


# ---------------------------------------------------------------------------------------------------------------
# group 6: the grid-stride loop of the fixed-shape kernels
# ---------------------------------------------------------------------------------------------------------------
def check_grid_stride(backend, n, src_shape, dst_shape, first_pass):
    """`n` sources whose 4 ny nx n output elements are more than the `first_pass` elements one pass of the grid
    covers: up to 64 items spread over the batch -- the first, the last, the ones either side of element
    `first_pass` -- equal the same items run as a batch of their own.  Returns the items compared."""
    rng = np.random.default_rng(606)
    sny, snx = src_shape
    ny, nx = dst_shape
    per = 4 * ny * nx
    assert n * per > first_pass
    src = rng.normal(size=(n, sny, snx)).astype(np.float32)
    k = np.arange(n)
    aff = np.zeros((n, 6))
    aff[:, 0] = aff[:, 4] = 0.5
    aff[:, 1] = 0.0625
    aff[:, 2] = (k % 8) / 8.0 - 1.0
    aff[:, 5] = (k % 5) / 8.0 - 0.5
    coef = affine_to_coef(aff, dst_shape)
    coef[:, 0, slot(2, 0)] = coef[:, 1, slot(1, 1)] = 2.0 ** -7
    b0 = first_pass // per
    picks = set(np.linspace(0, n - 1, min(n, 61)).astype(int).tolist()) | {0, n - 1}
    picks |= {b for b in (b0 - 1, b0, b0 + 1) if 0 <= b < n}
    picks = np.array(sorted(picks))
    assert len(picks) <= 64 and picks[0] == 0 and picks[-1] == n - 1 and b0 - 1 in picks and b0 in picks
    for kernel in ('affine', 'poly'):
        if kernel == 'affine':
            full = backend.affine(src, aff, dst_shape, None)
            part = backend.affine(src[picks], aff[picks], dst_shape, None)
        else:
            full = backend.poly(src, coef, 2, dst_shape, None)
            part = backend.poly(src[picks], coef[picks], 2, dst_shape, None)
        assert full.shape == (n, 4, ny, nx)
        bad = [int(b) for b, f, p in zip(picks, full[picks], part) if not np.array_equal(f, p)]
        assert not bad, (kernel, bad)
        assert all(p.any() for p in part), kernel
    return picks


# ---------------------------------------------------------------------------------------------------------------
# group 7: a NaN in the source stays local
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def group7():
    """12x12 normal fields with ONE NaN each -- in the interior, in the first column (which the continuation
    mirrors about), in the last row but one -- at unit scale on eighths and at scale 1/2"""
    rng = np.random.default_rng(607)
    cases = []
    for name, aff, shape in (('unit', [1, 0, -0.875, 0, 1, -1], (14, 14)),
                             ('half', [0.5, 0.125, -3.5, 0, 0.5, -0.5], (26, 28))):
        src = rng.normal(size=(3, 12, 12)).astype(np.float32)
        src[0, 5, 6] = src[1, 4, 0] = src[2, 10, 7] = np.nan
        cases.append(Case('nan ' + name, src, shape, np.array([aff] * 3, dtype=np.float64)))
    return tuple(cases)


def check_group7(backend, kernel):
    cases = group7()
    for case, got in zip(cases, run_cases(backend, kernel, cases)):
        hit = np.isnan(case.exp)
        # the NaN reaches the outputs whose continued 6x6 patch holds it and no others: some, not all
        for b in range(len(case.src)):
            assert 0 < hit[b].sum() < case.inside[b].sum(), (case.name, b)
        assert not hit[~case.inside].any()
        differ = np.argwhere(np.isnan(got) != hit)
        assert differ.size == 0, (case.name, kernel, differ[:8].tolist())
        check_bound(got, case, kernel)
