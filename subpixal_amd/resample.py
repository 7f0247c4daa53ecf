"""Drizzle of dithered frames on the device, with the leave-one-out interface of the reference's ``Resample``
(subpixal/resample.py) where that has a meaning without files, WCS objects and drizzlepac.

``DeviceDrizzle`` holds K frames (CUDA tensors), one forward map per frame -- input pixel -> output pixel, either
affine, ``(X, Y) = (a0 x + a1 y + a2, a3 x + a4 y + a5)``, the ``[6]`` layout of ``blot.shift_affine``, or a
:class:`PolyMap`, a bivariate polynomial of degree 1 .. 5 (instrument distortion) -- and a fixed output grid.
``execute()`` is one launch of the gather kernel of csrc/spx_drizzle_kernels.h (``spx_drizzle_f32`` / ``_f64``);
include/subpixal_hip.h carries the definition in full.  ``output_sci`` is the weighted MEAN of the input
values that land on a pixel, i.e. input-pixel surface brightness: no ``scale**2`` is applied when the map changes the
pixel area.  drizzlepac is not in the reference tree, so parity with it is UNPINNED (the definition is this
library's own, after Fruchter & Hook 2002); FITS input/output is not here.

Sky subtraction (``skysub=True``; off by default, and with it off nothing differs: no new tensor, no new launch, the
same row bytes) stands where the reference runs ``sky.subtractSky`` (resample.py:359-364): the first full
``execute()`` computes every listed frame's sigma-clipped level in one call of ``sky.frame_stats``'s kernels
(csrc/spx_sky_kernels.h) over the frame's own mask and weight, keeps it as ``computed_sky`` and FREEZES it, as the
reference's sky file does for its leave-one-out drizzles (resample.py:586-597).  The drizzle, the median, the
comparison and ``crclean`` then read ``frame - T(sky)``, one IEEE subtraction in the frame's dtype made on the device
into a second tensor (``science(name)``); the frame as given is kept.  The definition is the library's own
(include/subpixal_hip.h, sky block), parity with drizzlepac UNPINNED; its ``'match'`` methods, the static mask and
its histogram mode are not here.

With at least one ``PolyMap`` among the maps every row is packed by ``spx_drizzle_poly_rows`` (an affine entry
becomes a degree-1 row) and ``execute()`` launches the gather of csrc/spx_drizzle_poly_kernels.h
(``spx_drizzle_poly_f32`` / ``_f64``); with none nothing differs from the affine path, bit for bit.  Cosmic-ray
rejection is not there for polynomial maps yet (its median and blot kernels read affine rows): ``cr_reject=True``
together with a ``PolyMap`` is a ValueError.

Cosmic-ray rejection (``cr_reject=True``; off by default, and with it off nothing differs from the plain drizzle) runs
the steps of the reference's full ``execute()`` (resample.py:366-390) on the device: the median of the single-frame
drizzles (``spx_drizzle_median_*``), per frame the blot of that median, its derivative and the two-threshold
comparison (``spx_drizzle_cr_*``), then the final drizzle with every frame's mask merged with its cosmic-ray mask.
The definition is again the library's own, modelled on drizzlepac's createMedian / ablot / quickDeriv / drizCR and
written out in include/subpixal_hip.h; parity with drizzlepac is UNPINNED.

A visit of two or three exposures is what the median cannot clean: with K = 2 it is the mean, carries half of every
hit and makes the comparison flag the clean frame as well.  ``combine_type='minmed'`` (``spx_drizzle_minmed_*``, step
2' of the header) takes the minimum of the single-frame drizzles where the median stands ``combine_nsigma`` of the
minimum's own noise above it, and around such pixels (``combine_grow``); ``driz_cr_grow`` and ``driz_cr_ctegrow`` /
``driz_cr_ctedir`` (``spx_drizzle_cr_grow_*``, step 7) grow every frame's mask by a block and along the readout
direction, so that a hit's faint wings do not stay in ``crclean``.  Modelled on drizzlepac's keywords of the same
names, the definition the library's own, parity UNPINNED.  With every one of these keywords at its default
``execute()`` makes exactly the calls it made without them.  The other combine types and static masks are not here.

The per-frame table the kernel reads lives on the device; ``set_map`` and dropping or adding a frame rewrite one
row.  Dropping only clears the frame's ``active`` flag, so the result is bit-identical to a fresh drizzle of the
remaining frames in list order (``output_ctx`` numbers its bits by ``table_names``, dropped frames included).
"""
from fractions import Fraction

import numpy as np

from . import _ffi

__all__ = ['DeviceDrizzle', 'PolyMap', 'KERNELS', 'MAX_FRAMES', 'MAX_DEGREE', 'POLY_TERMS']

KERNELS = {'square': 0, 'turbo': 1, 'point': 2}            # SPX_DRIZZLE_SQUARE / _TURBO / _POINT
_ROW_MASK = 16                                             # byte offset of a packed row's mask pointer (its third field)
MAX_FRAMES = 128
MAX_DEGREE = 5                                             # of a PolyMap
POLY_TERMS = 21                                            # monomials u^i v^j with i + j <= 5 (blot.POLY_TERMS)
_DTYPES = ('float32', 'float64')


def _dtype_name(a):
    return str(a.dtype).replace('torch.', '')


def _slot(i, j):
    """the slot of u^i v^j among the 21: k = d (d + 1) / 2 + (d - i), d = i + j (``spx_blot_poly4_f32``)"""
    return (i + j) * (i + j + 1) // 2 + j


_TERMS = [(d - j, j) for d in range(MAX_DEGREE + 1) for j in range(d + 1)]          # (i, j) of slot 0 .. 20


def _pmul(p, q):
    out = {}
    for (i, j), a in p.items():
        for (k, l), b in q.items():
            out[i + k, j + l] = out.get((i + k, j + l), 0) + a * b
    return out


def _substitute(coef, degree, lu, lv):
    """The coefficients [2, 21] of P(lu(u', v'), lv(u', v')) for the linear forms ``lu = (a, b, e)`` meaning
    a u' + b v' + e (``lv`` likewise), in exact rational arithmetic: each result is rounded once."""
    lu = {(1, 0): Fraction(lu[0]), (0, 1): Fraction(lu[1]), (0, 0): Fraction(lu[2])}
    lv = {(1, 0): Fraction(lv[0]), (0, 1): Fraction(lv[1]), (0, 0): Fraction(lv[2])}
    pu, pv = [{(0, 0): Fraction(1)}], [{(0, 0): Fraction(1)}]
    for _ in range(degree):
        pu.append(_pmul(pu[-1], lu))
        pv.append(_pmul(pv[-1], lv))
    out = np.zeros((2, POLY_TERMS))
    mono = {}
    for axis in range(2):
        acc = {}
        for k, (i, j) in enumerate(_TERMS):
            if i + j > degree or coef[axis, k] == 0.0:
                continue
            if (i, j) not in mono:
                mono[i, j] = _pmul(pu[i], pv[j])
            c = Fraction(float(coef[axis, k]))
            for key, val in mono[i, j].items():
                acc[key] = acc.get(key, 0) + c * val
        for (i, j), val in acc.items():
            out[axis, _slot(i, j)] = float(val)
    return out


class PolyMap(object):
    """``PolyMap(coef, degree, center=(0.0, 0.0))``: a forward map input pixel -> output pixel that is a bivariate
    polynomial of total degree ``degree`` (1 .. 5) in ``u = x - xc, v = y - yc``,
    ``X = sum_d sum_{i=d..0} coef[0][k] u^i v^(d-i)``, ``k = d (d + 1) / 2 + (d - i)``, ``Y`` with ``coef[1]``: the term
    order and the 21 slots of ``spx_blot_poly4_f32`` / ``blot.poly_from_map``.  An immutable value object, host
    float64 only; slots above ``degree`` are cleared."""
    __slots__ = ('_coef', '_degree', '_center')

    def __init__(self, coef, degree, center=(0.0, 0.0)):
        if int(degree) != degree or not 1 <= int(degree) <= MAX_DEGREE:
            raise ValueError("maps: the degree of a polynomial map must be 1 .. %d, got %r." % (MAX_DEGREE, degree))
        degree = int(degree)
        c = np.array(coef, dtype=np.float64)
        n = (degree + 1) * (degree + 2) // 2
        if c.ndim != 2 or c.shape[0] != 2 or not n <= c.shape[1] <= POLY_TERMS:
            raise ValueError("maps: the coefficients of a polynomial map must have shape (2, 21), got %s."
                             % (c.shape,))
        full = np.zeros((2, POLY_TERMS))
        full[:, :n] = c[:, :n]
        center = np.array(center, dtype=np.float64)
        if center.shape != (2,) or not np.all(np.isfinite(center)) or not np.all(np.isfinite(full)):
            raise ValueError("maps: the coefficients and the centre of a polynomial map must be finite.")
        full.setflags(write=False)
        center.setflags(write=False)
        object.__setattr__(self, '_coef', full)
        object.__setattr__(self, '_degree', degree)
        object.__setattr__(self, '_center', center)

    def __setattr__(self, name, value):
        raise AttributeError("PolyMap is immutable.")

    coef = property(lambda self: self._coef)
    degree = property(lambda self: self._degree)
    center = property(lambda self: self._center)

    def __repr__(self):
        return 'PolyMap(degree=%d, center=(%r, %r))' % (self._degree, self._center[0], self._center[1])

    def _sum(self, x, y, du=0, dv=0):
        u = np.asarray(x, dtype=np.float64) - self._center[0]
        v = np.asarray(y, dtype=np.float64) - self._center[1]
        out = [np.zeros(np.broadcast(u, v).shape), np.zeros(np.broadcast(u, v).shape)]
        for k, (i, j) in enumerate(_TERMS):
            if i + j > self._degree or i < du or j < dv:
                continue
            f = (i if du else 1) * (j if dv else 1)
            term = f * u ** (i - du) * v ** (j - dv)
            out[0] = out[0] + self._coef[0, k] * term
            out[1] = out[1] + self._coef[1, k] * term
        return out[0], out[1]

    def __call__(self, x, y):
        """``(X, Y)`` of the input positions ``(x, y)`` (arrays)"""
        return self._sum(x, y)

    def jacobian(self, x, y):
        """``[..., 2, 2]``: ``[[dX/dx, dX/dy], [dY/dx, dY/dy]]`` at ``(x, y)``"""
        xu, yu = self._sum(x, y, du=1)
        xv, yv = self._sum(x, y, dv=1)
        return np.stack([np.stack([xu, xv], axis=-1), np.stack([yu, yv], axis=-1)], axis=-2)

    def inverse(self, X, Y, tol=1e-12, max_iter=50):
        """``(x, y)`` with ``M(x, y) = (X, Y)`` by Newton from the linearisation at the centre, to ``tol`` px -- or to
        16 ulps of the largest coordinate in play where that is more (7e-12 px at 4096): a float64 evaluation cannot
        tell positions closer than that apart.  Raises ValueError if it does not converge."""
        X, Y = np.broadcast_arrays(np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64))
        a = self.affine()
        det = a[0] * a[4] - a[1] * a[3]
        x = (a[4] * (X - a[2]) - a[1] * (Y - a[5])) / det
        y = (-a[3] * (X - a[2]) + a[0] * (Y - a[5])) / det
        for _ in range(int(max_iter)):
            fx, fy = self(x, y)
            j = self.jacobian(x, y)
            d = j[..., 0, 0] * j[..., 1, 1] - j[..., 0, 1] * j[..., 1, 0]
            rx, ry = fx - X, fy - Y
            with np.errstate(all='ignore'):
                dx = (j[..., 1, 1] * rx - j[..., 0, 1] * ry) / d
                dy = (-j[..., 1, 0] * rx + j[..., 0, 0] * ry) / d
            x, y = x - dx, y - dy
            step = max(float(np.max(np.abs(dx), initial=0.0)), float(np.max(np.abs(dy), initial=0.0)))
            if not np.isfinite(step):
                break
            size = max(float(np.max(np.abs(x), initial=1.0)), float(np.max(np.abs(y), initial=1.0)),
                       float(np.max(np.abs(X), initial=1.0)), float(np.max(np.abs(Y), initial=1.0)))
            if step <= max(tol, 16.0 * 2.0 ** -53 * size):
                return x, y
        raise ValueError("PolyMap.inverse: Newton's iteration did not converge to %g px." % tol)

    def affine(self):
        """the ``[6]`` linearisation at the centre"""
        c, (xc, yc) = self._coef, self._center
        return np.array([c[0, 1], c[0, 2], c[0, 0] - c[0, 1] * xc - c[0, 2] * yc,
                         c[1, 1], c[1, 2], c[1, 0] - c[1, 1] * xc - c[1, 2] * yc])

    def about(self, center):
        """the same map re-expanded about another centre: exact rational arithmetic, each coefficient rounded once"""
        center = np.asarray(center, dtype=np.float64)
        sx = Fraction(float(center[0])) - Fraction(float(self._center[0]))
        sy = Fraction(float(center[1])) - Fraction(float(self._center[1]))
        return PolyMap(_substitute(self._coef, self._degree, (1, 0, sx), (0, 1, sy)), self._degree, center)

    def compose(self, affine6):
        """``M o G`` for the affine ``G(p) = (g0 x + g1 y + g2, g3 x + g4 y + g5)`` on the input side: a polynomial
        of the same degree about the centre ``G^-1(centre)``, re-expanded exactly."""
        g = np.asarray(affine6, dtype=np.float64)
        if g.shape != (6,) or not np.all(np.isfinite(g)) or g[0] * g[4] - g[1] * g[3] == 0.0:
            raise ValueError("compose: an invertible affine of six finite numbers.")
        det = g[0] * g[4] - g[1] * g[3]
        xc, yc = self._center
        nc = np.array([(g[4] * (xc - g[2]) - g[1] * (yc - g[5])) / det, (-g[3] * (xc - g[2]) + g[0] * (yc - g[5])) / det])
        f = [Fraction(float(v)) for v in g]
        # u = G(p)_x - xc = g0 u' + g1 v' + (g0 nx + g1 ny + g2 - xc), the last term the rounding of the new centre
        ex = f[0] * Fraction(float(nc[0])) + f[1] * Fraction(float(nc[1])) + f[2] - Fraction(float(xc))
        ey = f[3] * Fraction(float(nc[0])) + f[4] * Fraction(float(nc[1])) + f[5] - Fraction(float(yc))
        return PolyMap(_substitute(self._coef, self._degree, (f[0], f[1], ex), (f[3], f[4], ey)), self._degree, nc)

    @classmethod
    def from_affine(cls, a6, center=(0.0, 0.0)):
        a = np.asarray(a6, dtype=np.float64)
        if a.shape != (6,):
            raise ValueError("maps: an affine map is six numbers (a0 a1 a2 a3 a4 a5).")
        xc, yc = float(center[0]), float(center[1])
        coef = np.zeros((2, POLY_TERMS))
        coef[0, :3] = (a[0] * xc + a[1] * yc) + a[2], a[0], a[1]
        coef[1, :3] = (a[3] * xc + a[4] * yc) + a[5], a[3], a[4]
        return cls(coef, 1, (xc, yc))

    @classmethod
    def fit(cls, mapping, shape, degree=3, center=None):
        """Least-squares fit of any callable ``(x, y) -> (X, Y)`` over a frame of ``shape = (ny, nx)``, about
        ``center`` (default: the frame's centre).  Returns ``(map, max_residual_px)``; as ``blot.poly_from_map`` the
        residual is taken on a finer probe grid (25 x 25 over the pixels' full extent) than the fit uses (17 x 17)."""
        degree = int(degree)
        if not 1 <= degree <= MAX_DEGREE:
            raise ValueError("degree must be 1 .. %d." % MAX_DEGREE)
        ny, nx = int(shape[0]), int(shape[1])
        xc, yc = (0.5 * (nx - 1), 0.5 * (ny - 1)) if center is None else (float(center[0]), float(center[1]))
        scale = 0.5 * max(nx, ny)                          # the design in u / scale: conditioned whatever the size

        def grid(k):
            gx, gy = np.meshgrid(np.linspace(-0.5, nx - 0.5, k), np.linspace(-0.5, ny - 0.5, k))
            return gx.ravel(), gy.ravel()

        def design(gx, gy):
            u, v = (gx - xc) / scale, (gy - yc) / scale
            return np.stack([u ** i * v ** j for i, j in _TERMS if i + j <= degree], axis=1)

        gx, gy = grid(17)
        X, Y = mapping(gx, gy)
        dm = design(gx, gy)
        cx, *_ = np.linalg.lstsq(dm, np.asarray(X, dtype=np.float64), rcond=None)
        cy, *_ = np.linalg.lstsq(dm, np.asarray(Y, dtype=np.float64), rcond=None)
        unscale = np.array([scale ** -(i + j) for i, j in _TERMS if i + j <= degree])
        m = cls(np.stack([cx * unscale, cy * unscale]), degree, (xc, yc))
        px, py = grid(25)
        PX, PY = mapping(px, py)
        mx, my = m(px, py)
        return m, float(np.hypot(mx - PX, my - PY).max())


def _is_poly(m):
    return isinstance(m, PolyMap)


def _check_map(m, what):
    if _is_poly(m):
        return m                                           # immutable, and checked when it was made
    m = np.asarray(m, dtype=np.float64)
    if m.shape != (6,) or not np.all(np.isfinite(m)):
        raise ValueError("maps: the map of %s must be six finite numbers (a0 a1 a2 a3 a4 a5)." % what)
    if m[0] * m[4] - m[1] * m[3] == 0.0:
        raise ValueError("maps: the map of %s is singular." % what)
    return m.copy()


class _Frame(object):
    """one frame of the pool: data, weight and mask as given (numpy or torch) until they are made resident"""
    __slots__ = ('data', 'weight', 'mask', 'resident')

    def __init__(self, data, weight, mask):
        self.data, self.weight, self.mask, self.resident = data, weight, mask, False


class DeviceDrizzle(object):
    """``DeviceDrizzle(frames, maps, out_shape, names=None, weights=None, masks=None, pixfrac=1.0, kernel='square',
    fill=0.0)``

    frames : sequence of K (1..128) 2-D arrays or tensors, all float32 or all float64; shapes may differ.
    maps : ``[K, 6]`` forward affine maps, input pixel -> output pixel (0-based, pixel centres on integers), or a
        sequence of K entries, each a ``[6]`` array or a :class:`PolyMap`.
    out_shape : ``(NY, NX)`` of the output grid (``reference_image``); it never changes.
    names : K distinct hashable names (default ``0 .. K-1``).
    weights : None, or per frame None (weight 1) or a map of the frame's shape, >= 0; a pixel that is masked, not
        finite, or whose weight is not finite or <= 0 does not contribute.
    masks : None, or per frame None or a bad-pixel mask of the frame's shape (nonzero / True = bad).
    pixfrac in (0, 1], kernel 'square' | 'turbo' | 'point', fill: the value of ``output_sci`` where nothing lands.
    cr_reject : reject cosmic rays in every full ``execute()`` (default False).  It needs
    rms : the frames' noise: one scalar for all, or per frame a scalar or a map of the frame's shape.
    gain, sky : None, a scalar, or one scalar per frame: ``var = rms**2 + max(blot - sky, 0) / gain`` (no gain: no
        Poisson term).
    combine_nlow, combine_nhigh : values dropped from the median at either end where that leaves one.
    driz_cr_snr, driz_cr_scale : the two thresholds, ``(3.5, 3.0)`` and ``(1.2, 0.7)``; the second pair must not exceed
        the first.
    combine_type : 'median' (default) or 'minmed'.  combine_nsigma : minmed's two thresholds, ``(4.0, 3.0)``.
    combine_grow : 0 .. 8, the reach of minmed's neighbour rule (default 1).
    combine_rms : minmed's noise of a single-frame drizzle, a scalar or one per frame; default: the frame's ``rms``
        where that is a scalar.
    driz_cr_grow : odd, 1 .. 9: every rejected pixel flags the testable pixels of the block around it (default 1:
        none).  driz_cr_ctegrow : 0 .. 64, and driz_cr_ctedir, a scalar or one per frame, each -1, 0 or +1: the
        pixels ``(i, j + ctedir tau)``, tau = 1 .. ctegrow, behind a rejected pixel ``(i, j)`` are flagged too.
        ``crmask(name)`` is the grown mask, ``crseed(name)`` the mask before the growth; ``output_minmed`` (uint8: 0
        median, 1 minimum, 2 minimum by the neighbour rule) is None unless minmed ran.
    skysub : subtract each frame's sky level before everything else (default False).  With it ``sky`` must stay None.
    skystat ('median' | 'mean' | 'mode'), skylower, skyupper, skyclip, skylsigma, skyusigma : the statistics, as
        ``sky.frame_stats``'s ``stat, lower, upper, clip, lsigma, usigma``.
    skymethod : 'localmin' (each frame its own level) or 'globalmin' (the lowest of them for all).
    skyuser : None, or one scalar per frame: the levels to subtract; nothing is computed then.
    ``computed_sky`` holds the levels once they exist; they are frozen until it is assigned or a ``sky*`` keyword
    changes.
    ``set_config_parameters`` takes the same keywords; per-frame values are in the order of ``names``.

    Nothing touches the device before ``execute()``; argument errors are ValueErrors raised here."""

    def __init__(self, frames, maps, out_shape, names=None, weights=None, masks=None, pixfrac=1.0, kernel='square',
                 fill=0.0, cr_reject=False, rms=None, gain=None, sky=None, combine_nlow=0, combine_nhigh=0,
                 driz_cr_snr=(3.5, 3.0), driz_cr_scale=(1.2, 0.7), skysub=False, skystat='median', skymethod='localmin',
                 skylower=None, skyupper=None, skyclip=5, skylsigma=4.0, skyusigma=4.0, skyuser=None,
                 combine_type='median', combine_nsigma=(4.0, 3.0), combine_grow=1, combine_rms=None, driz_cr_grow=1,
                 driz_cr_ctegrow=0, driz_cr_ctedir=0):
        frames = list(frames)
        K = len(frames)
        if not 1 <= K <= MAX_FRAMES:
            raise ValueError("frames: 1 .. %d frames, got %d." % (MAX_FRAMES, K))
        names = list(range(K)) if names is None else list(names)
        if len(names) != K or len(set(names)) != K:
            raise ValueError("names: one distinct name per frame.")
        if not isinstance(maps, np.ndarray) and any(_is_poly(m) for m in maps):
            maps = list(maps)
            if len(maps) != K:
                raise ValueError("maps: expected %d maps, got %d." % (K, len(maps)))
        else:
            maps = np.asarray(maps, dtype=np.float64)
            if maps.shape != (K, 6):
                raise ValueError("maps: expected shape (%d, 6), got %s." % (K, maps.shape))
        weights = K * [None] if weights is None else list(weights)
        masks = K * [None] if masks is None else list(masks)
        if len(weights) != K:
            raise ValueError("weights: one entry (or None) per frame.")
        if len(masks) != K:
            raise ValueError("masks: one entry (or None) per frame.")
        dt = _dtype_name(frames[0])
        if dt not in _DTYPES:
            raise ValueError("frames: dtype must be float32 or float64, got %s." % dt)
        for k, f in enumerate(frames):
            if len(f.shape) != 2 or min(f.shape) < 1 or _dtype_name(f) != dt:
                raise ValueError("frames: frame %r must be 2-D, not empty and %s like frame %r."
                                 % (names[k], dt, names[0]))
            if weights[k] is not None and tuple(weights[k].shape) != tuple(f.shape):
                raise ValueError("weights: the weight map of frame %r has shape %s, the frame %s."
                                 % (names[k], tuple(weights[k].shape), tuple(f.shape)))
            if masks[k] is not None and tuple(masks[k].shape) != tuple(f.shape):
                raise ValueError("masks: the mask of frame %r has shape %s, the frame %s."
                                 % (names[k], tuple(masks[k].shape), tuple(f.shape)))
        out_shape = tuple(int(n) for n in out_shape)
        if len(out_shape) != 2 or min(out_shape) < 1 or out_shape[0] * out_shape[1] >= 2 ** 31 - 1:
            raise ValueError("out_shape: (NY, NX) with 1 .. 2^31 - 2 pixels.")
        self._dtype = dt
        self._out_shape = out_shape
        self._pool = {n: _Frame(f, w, m) for n, f, w, m in zip(names, frames, weights, masks)}
        self._maps = {n: _check_map(m, repr(n)) for n, m in zip(names, maps)}
        self._order = list(names)                      # the table's rows: every frame ever listed, dropped ones too
        self._active = {n: True for n in names}
        self._pixfrac, self._kernel, self._fill = 1.0, 'square', 0.0
        self._names0 = list(names)                     # the order per-frame configuration values are given in
        self._cr = dict(on=False, rms=None, gain=None, sky=None, nlow=0, nhigh=0, snr=(3.5, 3.0), scale=(1.2, 0.7),
                        combine='median', nsigma=(4.0, 3.0), combine_grow=1, combine_rms=None, grow=1, ctegrow=0,
                        ctedir={n: 0 for n in names})
        self._rms_dev = {}                             # name -> the resident rms map
        self._crmask, self._merged, self._crclean = {}, {}, {}
        self._crseed = {}                              # name -> the mask before step 7 grew it
        self._fast = False                             # execute() was called by fast_replace_image
        self._skycfg = dict(on=False, stat='median', method='localmin', lower=None, upper=None, clip=5, lsigma=4.0,
                            usigma=4.0, user=None)
        self._sky = {}                                 # name -> the frozen sky value (``computed_sky``)
        self._sky_global = None                        # 'globalmin': the lowest of the first computation
        self._sub = {}                                 # name -> (sky value, frame - sky on the device)
        self.set_config_parameters(pixfrac=pixfrac, kernel=kernel, fill=fill, cr_reject=cr_reject, rms=rms, gain=gain,
                                   sky=sky, combine_nlow=combine_nlow, combine_nhigh=combine_nhigh,
                                   driz_cr_snr=driz_cr_snr, driz_cr_scale=driz_cr_scale, skysub=skysub,
                                   skystat=skystat, skymethod=skymethod, skylower=skylower, skyupper=skyupper,
                                   skyclip=skyclip, skylsigma=skylsigma, skyusigma=skyusigma, skyuser=skyuser,
                                   combine_type=combine_type, combine_nsigma=combine_nsigma, combine_grow=combine_grow,
                                   combine_rms=combine_rms, driz_cr_grow=driz_cr_grow, driz_cr_ctegrow=driz_cr_ctegrow,
                                   driz_cr_ctedir=driz_cr_ctedir)
        self._rows_host = None                         # uint8 [K][ROW_BYTES], as spx_drizzle_rows packed them
        self._rows_dev = None
        self._rows_poly = False                        # the rows are spx_drizzle_poly_rows' (a PolyMap among the maps)
        self._stale = True                             # the whole table must be packed again
        self.output_sci = self.output_wht = self.output_ctx = None
        self.output_median = self.output_nmedian = self.output_crmask = self.output_crclean = None
        self.output_minmed = None

    # ------------------------------------------------------------------------------------------------------
    # the reference's Resample interface
    # ------------------------------------------------------------------------------------------------------
    @property
    def input_image_names(self):
        """the frames the next ``execute()`` combines, in list order"""
        return [n for n in self._order if self._active[n]]

    @property
    def table_names(self):
        """the name of every row of the device table: bit k of ``output_ctx`` belongs to ``table_names[k]``"""
        return list(self._order)

    @property
    def reference_image(self):
        """the fixed output grid, ``(NY, NX)``"""
        return self._out_shape

    @property
    def dtype(self):
        return np.dtype(self._dtype)

    def set_config_parameters(self, pixfrac=None, kernel=None, fill=None, cr_reject=None, rms=None, gain=None,
                              sky=None, combine_nlow=None, combine_nhigh=None, driz_cr_snr=None, driz_cr_scale=None,
                              skysub=None, skystat=None, skymethod=None, skylower=None, skyupper=None, skyclip=None,
                              skylsigma=None, skyusigma=None, skyuser=None, combine_type=None, combine_nsigma=None,
                              combine_grow=None, combine_rms=None, driz_cr_grow=None, driz_cr_ctegrow=None,
                              driz_cr_ctedir=None):
        if pixfrac is not None:
            pixfrac = float(pixfrac)
            if not 0.0 < pixfrac <= 1.0:
                raise ValueError("pixfrac must lie in (0, 1], got %r." % pixfrac)
            self._pixfrac = pixfrac
        if kernel is not None:
            if kernel not in KERNELS:
                raise ValueError("kernel must be one of %s, got %r." % (sorted(KERNELS), kernel))
            self._kernel = kernel
        if fill is not None:
            fill = float(fill)
        cr = dict(self._cr)
        if rms is not None:
            cr['rms'] = self._per_frame(rms, 'rms', maps=True)
        if gain is not None:
            cr['gain'] = self._per_frame(gain, 'gain')
        if sky is not None:
            cr['sky'] = self._per_frame(sky, 'sky')
            if not all(np.isfinite(v) for v in cr['sky'].values()):
                raise ValueError("sky must be finite.")
        for key, val in (('nlow', combine_nlow), ('nhigh', combine_nhigh)):
            if val is not None:
                if int(val) != val or val < 0:
                    raise ValueError("combine_%s must be an integer >= 0, got %r." % (key, val))
                cr[key] = int(val)
        for key, val in (('snr', driz_cr_snr), ('scale', driz_cr_scale)):
            if val is not None:
                try:
                    pair = tuple(float(v) for v in val)
                except TypeError:
                    pair = ()
                if len(pair) != 2 or not all(np.isfinite(v) and v >= 0 for v in pair) or pair[1] > pair[0]:
                    raise ValueError("driz_cr_%s must be two finite numbers >= 0, the second not above the first, "
                                     "got %r." % (key, val))
                cr[key] = pair
        self._minmed_parameters(cr, combine_type, combine_nsigma, combine_grow, combine_rms, driz_cr_grow,
                                driz_cr_ctegrow, driz_cr_ctedir)
        if cr_reject is not None:
            cr['on'] = bool(cr_reject)
        sk = self._sky_parameters(skysub, skystat, skymethod, skylower, skyupper, skyclip, skylsigma, skyusigma,
                                  skyuser)
        if sk['on'] and cr['sky'] is not None:
            raise ValueError("sky: with skysub the frames the comparison sees are sky-free (the sky's noise belongs "
                             "in rms): give skysub or sky, not both.")
        if cr['on']:
            self._no_poly_with_cr(self._maps.values())
            if cr['rms'] is None:
                raise ValueError("rms: cr_reject needs the frames' noise (a scalar, or per frame a scalar or a map).")
            if min(self._out_shape) < 6:
                raise ValueError("out_shape: cr_reject needs an output of 6 x 6 pixels at least (the blot's quintic).")
            if cr['combine'] == 'minmed' and cr['combine_rms'] is None:
                for n in self._names0:
                    if not isinstance(cr['rms'][n], float):
                        raise ValueError("combine_rms: 'minmed' needs one noise value per frame, and the rms of frame "
                                         "%r is a map: give combine_rms (a scalar, or one scalar per frame)." % (n,))
        if fill is not None:
            self._fill = fill
        if rms is not None:
            self._rms_dev = {}
        self._cr = cr
        if sk != self._skycfg:                         # a sky* keyword changed: the frozen values go
            self._skycfg = sk
            self._sky, self._sky_global, self._sub = {}, None, {}
        self._stale = True

    def _minmed_parameters(self, cr, combine_type, combine_nsigma, combine_grow, combine_rms, driz_cr_grow,
                           driz_cr_ctegrow, driz_cr_ctedir):
        """the minmed and growth keywords that are given (not None), checked, into the dict ``cr``"""
        if combine_type is not None:
            if combine_type not in ('median', 'minmed'):
                raise ValueError("combine_type must be 'median' or 'minmed', got %r." % (combine_type,))
            cr['combine'] = combine_type
        if combine_nsigma is not None:
            try:
                pair = tuple(float(v) for v in combine_nsigma)
            except TypeError:
                pair = ()
            if len(pair) != 2 or not all(np.isfinite(v) and v >= 0 for v in pair) or pair[1] > pair[0]:
                raise ValueError("combine_nsigma must be two finite numbers >= 0, the second not above the first, "
                                 "got %r." % (combine_nsigma,))
            cr['nsigma'] = pair
        for key, val, lo, hi, odd in (('combine_grow', combine_grow, 0, 8, False), ('grow', driz_cr_grow, 1, 9, True),
                                      ('ctegrow', driz_cr_ctegrow, 0, 64, False)):
            if val is not None:
                name = key if key == 'combine_grow' else 'driz_cr_' + key
                if len(getattr(val, 'shape', ())) != 0 or isinstance(val, (list, tuple)) or int(val) != val \
                        or not lo <= val <= hi or (odd and int(val) % 2 == 0):
                    raise ValueError("%s must be an%s integer %d .. %d, got %r." % (name, ' odd' if odd else '', lo, hi,
                                                                                   val))
                cr[key] = int(val)
        if combine_rms is not None:
            r = self._per_frame(combine_rms, 'combine_rms')
            if not all(np.isfinite(v) and v >= 0 for v in r.values()):
                raise ValueError("combine_rms must be finite and >= 0.")
            cr['combine_rms'] = r
        if driz_cr_ctedir is not None:
            r = self._per_frame(driz_cr_ctedir, 'driz_cr_ctedir')
            if not all(v in (-1.0, 0.0, 1.0) for v in r.values()):
                raise ValueError("driz_cr_ctedir: each entry must be -1, 0 or +1, got %r." % (driz_cr_ctedir,))
            cr['ctedir'] = {n: int(v) for n, v in r.items()}

    def _grows(self, name):
        """whether step 7 does anything for frame ``name``"""
        cr = self._cr
        return cr['grow'] > 1 or (cr['ctegrow'] > 0 and cr['ctedir'].get(name, 0) != 0)

    def _cr_entries(self):
        """the library entries a full ``execute()`` calls between its two drizzles, in order (without the dtype
        suffix): with every minmed and growth keyword at its default, the two it always called"""
        first = 'spx_drizzle_minmed' if self._cr['combine'] == 'minmed' else 'spx_drizzle_median'
        grows = any(self._grows(n) for n in self.input_image_names)
        return (first, 'spx_drizzle_cr') + (('spx_drizzle_cr_grow',) if grows else ())

    def _sky_parameters(self, skysub, skystat, skymethod, skylower, skyupper, skyclip, skylsigma, skyusigma, skyuser):
        """the ``sky*`` keywords that are given (not None) over the current ones, checked; nothing is stored"""
        from . import sky as _sky
        sk = dict(self._skycfg)
        given = dict(stat=skystat, method=skymethod, lower=skylower, upper=skyupper, clip=skyclip, lsigma=skylsigma,
                     usigma=skyusigma)
        sk.update({k: v for k, v in given.items() if v is not None})
        if skysub is not None:
            sk['on'] = bool(skysub)
        if sk['method'] not in ('localmin', 'globalmin'):
            raise ValueError("skymethod must be 'localmin' or 'globalmin', got %r." % (sk['method'],))
        try:
            stat, lower, upper, clip, lsigma, usigma = _sky.check_parameters(sk['stat'], sk['lower'], sk['upper'],
                                                                             sk['clip'], sk['lsigma'], sk['usigma'])
        except ValueError as e:
            raise ValueError('sky' + str(e))
        sk.update(clip=clip, lsigma=lsigma, usigma=usigma, lower=None if lower != lower else lower,
                  upper=None if upper != upper else upper)
        if skyuser is not None:
            sk['user'] = self._per_frame(skyuser, 'skyuser')
            if not all(np.isfinite(v) for v in sk['user'].values()):
                raise ValueError("skyuser must be finite.")
        return sk

    @property
    def computed_sky(self):
        """``{name: sky}`` of the frames that have a value (the reference's ``computed_sky``, resample.py:130-136):
        computed by the first full ``execute()`` with ``skysub`` and frozen from then on.  Assigning a dict replaces
        the values: the frames it names are subtracted by what it gives, the others get a value at the next
        ``execute()``."""
        return dict(self._sky)

    @computed_sky.setter
    def computed_sky(self, values):
        new = {}
        for n, v in dict(values).items():
            if n not in self._pool:
                raise ValueError("computed_sky: no frame named %r." % (n,))
            if len(getattr(v, 'shape', ())) != 0 or not np.isfinite(float(v)):
                raise ValueError("computed_sky: the value of frame %r must be a finite scalar." % (n,))
            new[n] = float(v)
        self._sky, self._sky_global, self._sub = new, None, {}
        self._stale = True

    def science(self, name):
        """the tensor of frame ``name`` the drizzle reads: ``frame - sky`` with ``skysub``, else the frame as given"""
        self._resident(name)
        return self._sci(name, want=True)

    def _per_frame(self, value, what, maps=False):
        """{name: value} from one scalar for all frames or one entry per frame, in the order of ``names``"""
        names = self._names0
        if not isinstance(value, (list, tuple)) and len(getattr(value, 'shape', ())) == 0:
            value = len(names) * [value]
        value = list(value)
        if len(value) != len(names):
            raise ValueError("%s: one scalar, or one entry per frame (%d), got %d." % (what, len(names), len(value)))
        out = {}
        for n, v in zip(names, value):
            if len(getattr(v, 'shape', ())) == 0:
                out[n] = float(v)
            elif maps:
                if tuple(v.shape) != tuple(self._pool[n].data.shape):
                    raise ValueError("%s: the map of frame %r has shape %s, the frame %s."
                                     % (what, n, tuple(v.shape), tuple(self._pool[n].data.shape)))
                out[n] = v
            else:
                raise ValueError("%s: the entry of frame %r must be a scalar." % (what, n))
        return out

    def crmask(self, name):
        """the cosmic-ray mask (uint8 CUDA tensor, 1 = rejected) the last full ``execute()`` made for frame ``name``,
        or None"""
        return self._crmask.get(name)

    def crseed(self, name):
        """the mask of frame ``name`` before ``driz_cr_grow`` / ``driz_cr_ctegrow`` grew it (``crmask(name)`` itself
        where nothing grew it), or None"""
        return self._crseed.get(name)

    def crclean(self, name):
        """frame ``name`` with its rejected pixels replaced by the blotted median (the reference's ``crclean_image``),
        or None when the last full ``execute()`` made none"""
        return self._crclean.get(name)

    @staticmethod
    def _no_poly_with_cr(maps):
        if any(_is_poly(m) for m in maps):
            raise ValueError("cr_reject: cosmic-ray rejection is not available for polynomial maps (PolyMap) yet: its "
                             "median and blot kernels read affine rows.")

    def _poly(self):
        return any(_is_poly(m) for m in self._maps.values())

    def map(self, name):
        """the map of frame ``name`` as it was set: a copy of the ``[6]`` array, or the (immutable) ``PolyMap``"""
        m = self._maps[name]
        return m if _is_poly(m) else m.copy()

    def set_map(self, name, affine):
        """Replace the map of frame ``name`` (listed or dropped) by a ``[6]`` affine or a ``PolyMap``; one row of the
        device table is rewritten (the whole table when the first ``PolyMap`` arrives or the last one leaves: the two
        kinds of row differ).  A map the packing refuses leaves everything as it was."""
        if name not in self._maps:
            raise ValueError("set_map: no frame named %r." % (name,))
        old = self._maps[name]
        new = _check_map(affine, repr(name))
        if self._cr['on']:
            self._no_poly_with_cr([new])
        self._maps[name] = new
        try:
            if self._poly() != self._rows_poly and self._rows_dev is not None and not self._stale:
                # the kind of row flips for EVERY frame, and the two packings size their windows differently: the
                # whole table is packed here, so that whatever is refused is refused before anything changes
                self._pack(self._order)
                self._stale = True
            else:
                self._rewrite_row(name)
        except ValueError:                             # what the packing refuses (the 8 x 8 window): nothing changes
            self._maps[name] = old
            raise

    def copy(self):
        """A second drizzle over the SAME resident frames with its own list, maps, tables and outputs (what the
        reference's loop takes a ``deepcopy`` for, align.py:272)."""
        c = object.__new__(DeviceDrizzle)
        c.__dict__.update(self.__dict__)
        c._pool = dict(self._pool)                     # the _Frame objects (and their tensors) are shared
        c._maps = {n: m if _is_poly(m) else m.copy() for n, m in self._maps.items()}
        c._order = list(self._order)
        c._active = dict(self._active)
        c._rows_host = None if self._rows_host is None else self._rows_host.copy()
        c._rows_dev = None if self._rows_dev is None else self._rows_dev.clone()
        c._cr = dict(self._cr)
        c._rms_dev = dict(self._rms_dev)
        # the sky values and the subtracted frames go along (shared tensors, own dicts)
        c._skycfg, c._sky, c._sub = dict(self._skycfg), dict(self._sky), dict(self._sub)
        # the cosmic-ray masks and the cleaned frames go along (shared tensors, own dicts)
        c._crmask, c._merged, c._crclean = dict(self._crmask), dict(self._merged), dict(self._crclean)
        c._crseed = dict(self._crseed)
        c.output_sci = c.output_wht = c.output_ctx = None
        return c

    def fast_drop_image(self, name):
        self.fast_replace_image(name, None)

    def fast_add_image(self, name):
        self.fast_replace_image(None, name)

    def fast_replace_image(self, drop=None, add=None):
        """resample.py:547-578, case by case: both None, or the same image: nothing happens; a ``drop`` that is not
        listed drops nothing; an ``add`` that is listed already is not added; an added image goes to the END of the
        list.  Then ``execute()``.  Images are added from the pool of every frame this object was built with or
        has dropped; a name it has never seen is a ValueError."""
        if drop is None and add is None:
            return
        if drop == add:
            return
        if add is not None and add not in self._pool:
            raise ValueError("fast_replace_image: no frame named %r was ever given to this drizzle." % (add,))
        if drop is not None and self._active.get(drop, False):
            self._active[drop] = False
            self._rewrite_row(drop)
        if add is not None and not self._active[add]:
            self._order.remove(add)
            self._order.append(add)
            self._active[add] = True
            self._stale = True                         # the rows change places
        # the median, the blot and the comparison are not run again (resample.py:604-606 switches them off): the
        # frames keep the masks of the last full execute(), a frame without one its original mask
        self._fast = True
        try:
            self.execute()
        finally:
            self._fast = False

    # ------------------------------------------------------------------------------------------------------
    # the device side
    # ------------------------------------------------------------------------------------------------------
    def _resident(self, name):
        import torch
        from . import device
        f = self._pool[name]
        if not f.resident:
            tdt = torch.float32 if self._dtype == 'float32' else torch.float64
            f.data = device.to_device(f.data, tdt)
            f.weight = None if f.weight is None else device.to_device(f.weight, tdt)
            if f.mask is not None:
                m = f.mask if isinstance(f.mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(f.mask))
                f.mask = device.to_device(m != 0, torch.uint8)
            f.resident = True
        return f

    def _ensure_sky(self, names):
        """A frozen sky value and the subtracted tensor for each of ``names`` that lacks one: the values of
        ``skyuser``, else ONE statistics call over the frames without a value, each with its own mask and weight.
        'globalmin': the lowest value of the first such call, for every frame, also for one added later.  A frame
        without a usable pixel (it contributes nothing) gets 0.  Returns True when a tensor was made."""
        import torch
        from . import sky as _sky
        sk = self._skycfg
        todo = [n for n in names if n not in self._sky]
        if todo and sk['user'] is not None:
            for n in todo:
                self._sky[n] = sk['user'][n]
        elif todo and sk['method'] == 'globalmin' and self._sky_global is not None:
            for n in todo:
                self._sky[n] = self._sky_global
        elif todo:
            fr = [self._resident(n) for n in todo]
            st = _sky.stats_resident([f.data for f in fr], [f.weight for f in fr], [f.mask for f in fr], self._dtype,
                                     *_sky.check_parameters(sk['stat'], sk['lower'], sk['upper'], sk['clip'],
                                                            sk['lsigma'], sk['usigma']))
            vals = [float(v) if np.isfinite(v) else 0.0 for v in st.sky]
            if sk['method'] == 'globalmin':
                good = [float(v) for v in st.sky if np.isfinite(v)]
                self._sky_global = min(good) if good else 0.0
                vals = len(todo) * [self._sky_global]
            self._sky.update(zip(todo, vals))
        made = False
        for n in names:
            if n not in self._sub or self._sub[n][0] != self._sky[n]:
                f = self._resident(n)
                self._sub[n] = (self._sky[n], f.data - torch.tensor(self._sky[n], dtype=f.data.dtype,
                                                                     device=f.data.device))
                made = True
        return made

    def _sci(self, name, want=False):
        """the tensor the rows point at: the subtracted one with ``skysub`` (made here for a listed frame, or when
        ``want``), else the frame as given"""
        if self._skycfg['on']:
            if name not in self._sub and (want or self._active[name]):
                self._ensure_sky([name])
            if name in self._sub:
                return self._sub[name][1]
        return self._pool[name].data

    def _pack(self, names, original=False):
        """rows for ``names`` through the library's host entry (ValueError for what it refuses); with cosmic-ray
        rejection on and unless ``original``, a frame's mask is the merged one of the last full ``execute()``"""
        lib = _ffi.load()
        K = len(names)
        fr = [self._resident(n) for n in names]
        frames = np.array([self._sci(n).data_ptr() for n in names], np.uint64)
        weights = np.array([0 if f.weight is None else f.weight.data_ptr() for f in fr], np.uint64)
        mk = [f.mask if original or not self._cr['on'] or n not in self._merged else self._merged[n]
              for n, f in zip(names, fr)]
        masks = np.array([0 if m is None else m.data_ptr() for m in mk], np.uint64)
        shapes = np.array([tuple(f.data.shape) for f in fr], np.int32)
        active = np.array([self._active[n] for n in names], np.uint8)
        if self._poly():
            pm = [m if _is_poly(m) else PolyMap.from_affine(m) for m in (self._maps[n] for n in names)]
            coef = np.ascontiguousarray(np.stack([m.coef for m in pm]))
            degree = np.array([m.degree for m in pm], np.int32)
            center = np.ascontiguousarray(np.stack([m.center for m in pm]))
            rows = np.zeros((K, _ffi.DRIZZLE_POLY_ROW_BYTES), np.uint8)
            rc = lib.spx_drizzle_poly_rows(frames.ctypes.data, weights.ctypes.data, masks.ctypes.data,
                                           shapes.ctypes.data, coef.ctypes.data, degree.ctypes.data,
                                           center.ctypes.data, active.ctypes.data, K, self._pixfrac,
                                           KERNELS[self._kernel], self._out_shape[0], self._out_shape[1],
                                           rows.ctypes.data)
        else:
            maps = np.ascontiguousarray(np.stack([self._maps[n] for n in names]))
            rows = np.zeros((K, _ffi.DRIZZLE_ROW_BYTES), np.uint8)
            rc = lib.spx_drizzle_rows(frames.ctypes.data, weights.ctypes.data, masks.ctypes.data, shapes.ctypes.data,
                                      maps.ctypes.data, active.ctypes.data, K, self._pixfrac, KERNELS[self._kernel],
                                      self._out_shape[0], self._out_shape[1], rows.ctypes.data)
        if rc in (_ffi.E_ARG, _ffi.E_SHAPE):
            raise ValueError(lib.spx_last_error().decode())
        _ffi.check(rc)
        return rows

    def _rewrite_row(self, name):
        if self._stale or self._rows_dev is None:
            self._stale = True                         # nothing on the device yet: execute() packs everything
            return
        import torch
        k = self._order.index(name)
        row = self._pack([name])
        self._rows_host[k] = row[0]
        self._rows_dev[k].copy_(torch.from_numpy(row[0]))

    def execute(self):
        """Drizzle the listed frames: ``output_sci`` (frame dtype), ``output_wht`` (float32) and ``output_ctx``
        (int32 ``[ceil(K / 32), NY, NX]``, K = ``len(table_names)``) are new CUDA tensors after every call.

        With ``cr_reject`` a call from outside is the reference's full ``execute()``: it starts again from the
        original masks, and sets ``output_median`` (float32), ``output_nmedian`` (uint8), ``output_crmask`` and
        ``output_crclean`` (lists of CUDA tensors in ``input_image_names`` order; ``crmask(name)``,
        ``crclean(name)``) before the final drizzle over the merged masks.  The ``fast_*`` methods recompute none of
        these."""
        import torch
        from . import device
        device.init()
        lib = _ffi.load()
        K = len(self._order)
        NY, NX = self._out_shape
        if self._skycfg['on']:
            listed = self.input_image_names
            if listed and self._ensure_sky(listed):
                self._stale = True
        if self._cr['on'] and not self._fast:
            self._reject_cosmic_rays(lib)
        elif not self._cr['on'] and self._merged:
            self._crmask, self._merged, self._crclean = {}, {}, {}
            self._crseed = {}
            self._stale = True
        if self._stale or self._rows_dev is None or self._rows_poly != self._poly():
            self._rows_host = self._pack(self._order)
            self._rows_dev = torch.from_numpy(self._rows_host).cuda()
            self._rows_poly = self._poly()
            self._stale = False
        dev = self._rows_dev.device
        sci = torch.empty((NY, NX), dtype=torch.float32 if self._dtype == 'float32' else torch.float64, device=dev)
        wht = torch.empty((NY, NX), dtype=torch.float32, device=dev)
        ctx = torch.empty(((K + 31) // 32, NY, NX), dtype=torch.int32, device=dev)
        if self._rows_poly:
            fn = lib.spx_drizzle_poly_f32 if self._dtype == 'float32' else lib.spx_drizzle_poly_f64
        else:
            fn = lib.spx_drizzle_f32 if self._dtype == 'float32' else lib.spx_drizzle_f64
        _ffi.check(fn(self._rows_dev.data_ptr(), K, KERNELS[self._kernel], self._fill, NY, NX, sci.data_ptr(),
                      wht.data_ptr(), ctx.data_ptr(), device.stream_ptr()))
        self.output_sci, self.output_wht, self.output_ctx = sci, wht, ctx
        return self

    def _rms_of(self, name):
        """(scalar, resident map or None) of frame ``name``"""
        import torch
        from . import device
        r = self._cr['rms'][name]
        if isinstance(r, float):
            return r, None
        if name not in self._rms_dev:
            self._rms_dev[name] = device.to_device(r, torch.float32 if self._dtype == 'float32' else torch.float64)
        return 0.0, self._rms_dev[name]

    def _reject_cosmic_rays(self, lib):
        """The steps between the two drizzles of a full ``execute()``: the median over the rows with the ORIGINAL
        masks, one comparison launch per listed frame, the merged masks.  The rows are packed once: the final
        drizzle's table is the same rows with the mask pointers of the listed frames set to the merged masks.  With
        no frame listed there is nothing to reject: no masks, no cleaned frames and no median."""
        import torch
        from . import device
        cr = self._cr
        K = len(self._order)
        NY, NX = self._out_shape
        f32 = self._dtype == 'float32'
        active = self.input_image_names
        self._crmask, self._merged, self._crclean = {}, {}, {}
        self._crseed = {}
        if not active:
            self.output_median = self.output_nmedian = self.output_minmed = None
            self.output_crmask, self.output_crclean = [], []
            self._stale = True
            return
        host = self._pack(self._order, original=True)
        rows = torch.from_numpy(host).cuda()
        dev, stream = rows.device, device.stream_ptr()
        med = torch.empty((NY, NX), dtype=torch.float32, device=dev)
        nmed = torch.empty((NY, NX), dtype=torch.uint8, device=dev)
        minmed = None
        if cr['combine'] == 'minmed':
            # step 2': the table (combine_rms, sky, gain) per row, the median, the minimum and the decision bits in
            # planes of their own (no pass reads a plane it writes), then the neighbour rule
            table = np.zeros((K, 3))
            for k, name in enumerate(self._order):
                r = cr['combine_rms'][name] if cr['combine_rms'] is not None else cr['rms'][name]
                g = None if cr['gain'] is None else cr['gain'][name]
                table[k] = (r, 0.0 if cr['sky'] is None else cr['sky'][name],
                            g if g is not None and np.isfinite(g) and g > 0 else 0.0)
            table = torch.from_numpy(table).cuda()
            md, lo = torch.empty_like(med), torch.empty_like(med)
            bits, minmed = torch.empty_like(nmed), torch.empty_like(nmed)
            fn = lib.spx_drizzle_minmed_f32 if f32 else lib.spx_drizzle_minmed_f64
            _ffi.check(fn(rows.data_ptr(), K, len(active), KERNELS[self._kernel], cr['nlow'], cr['nhigh'],
                          table.data_ptr(), cr['nsigma'][0], cr['nsigma'][1], cr['combine_grow'], NY, NX, md.data_ptr(),
                          lo.data_ptr(), bits.data_ptr(), med.data_ptr(), nmed.data_ptr(), minmed.data_ptr(), stream))
        else:
            fn = lib.spx_drizzle_median_f32 if f32 else lib.spx_drizzle_median_f64
            _ffi.check(fn(rows.data_ptr(), K, len(active), KERNELS[self._kernel], cr['nlow'], cr['nhigh'], NY, NX,
                          med.data_ptr(), nmed.data_ptr(), stream))
        fn = lib.spx_drizzle_cr_f32 if f32 else lib.spx_drizzle_cr_f64
        fn_grow = lib.spx_drizzle_cr_grow_f32 if f32 else lib.spx_drizzle_cr_grow_f64
        host = host.copy()
        for name in active:
            f = self._pool[name]
            ny, nx = f.data.shape
            rs, rm = self._rms_of(name)
            gain = None if cr['gain'] is None else cr['gain'][name]
            sky = 0.0 if cr['sky'] is None else cr['sky'][name]         # with skysub: 0, the frames are sky-free
            mask = torch.empty((ny, nx), dtype=torch.uint8, device=dev)
            clean = torch.empty_like(f.data)
            _ffi.check(fn(rows.data_ptr(), K, self._order.index(name), ny, nx, med.data_ptr(), nmed.data_ptr(), NY, NX,
                          rs, None if rm is None else rm.data_ptr(), sky, float('nan') if gain is None else gain,
                          cr['snr'][0], cr['snr'][1], cr['scale'][0], cr['scale'][1], mask.data_ptr(),
                          clean.data_ptr(), stream))
            self._crseed[name] = mask
            if self._grows(name):
                # step 7 reads the seed mask and writes the grown one into a plane of its own
                grown = torch.empty_like(mask)
                _ffi.check(fn_grow(rows.data_ptr(), K, self._order.index(name), ny, nx, med.data_ptr(),
                                   nmed.data_ptr(), NY, NX, rs, None if rm is None else rm.data_ptr(),
                                   mask.data_ptr(), cr['grow'], cr['ctegrow'], cr['ctedir'].get(name, 0),
                                   grown.data_ptr(), clean.data_ptr(), stream))
                mask = grown
            self._crmask[name], self._crclean[name] = mask, clean
            self._merged[name] = mask if f.mask is None else (f.mask | mask)
            host[self._order.index(name), _ROW_MASK:_ROW_MASK + 8].view(np.uint64)[0] = self._merged[name].data_ptr()
        self.output_median, self.output_nmedian, self.output_minmed = med, nmed, minmed
        self.output_crmask = [self._crmask[n] for n in active]
        self.output_crclean = [self._crclean[n] for n in active]
        self._rows_host, self._rows_dev = host, torch.from_numpy(host).cuda()
        self._stale = False
