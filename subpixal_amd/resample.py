"""Drizzle of dithered frames on the device, with the leave-one-out interface of the reference's ``Resample``
(subpixal/resample.py) where that has a meaning without files, WCS objects and drizzlepac.

``DeviceDrizzle`` holds K frames (CUDA tensors), one forward affine map per frame -- input pixel -> output pixel,
``(X, Y) = (a0 x + a1 y + a2, a3 x + a4 y + a5)``, the ``[6]`` layout of ``blot.shift_affine`` -- and a fixed output
grid.  ``execute()`` is one launch of the gather kernel of csrc/spx_drizzle_kernels.h (``spx_drizzle_f32`` /
``_f64``); include/subpixal_hip.h carries the definition in full.  ``output_sci`` is the weighted MEAN of the input
values that land on a pixel, i.e. input-pixel surface brightness: no ``scale**2`` is applied when the map changes the
pixel area.  drizzlepac is not in the reference tree, so parity with it is UNPINNED (the definition is this
library's own, after Fruchter & Hook 2002); polynomial distortion, sky subtraction and FITS input/output are not
here.

Cosmic-ray rejection (``cr_reject=True``; off by default, and with it off nothing differs from the plain drizzle) runs
the steps of the reference's full ``execute()`` (resample.py:366-390) on the device: the median of the single-frame
drizzles (``spx_drizzle_median_*``), per frame the blot of that median, its derivative and the two-threshold
comparison (``spx_drizzle_cr_*``), then the final drizzle with every frame's mask merged with its cosmic-ray mask.
The definition is again the library's own, modelled on drizzlepac's createMedian / ablot / quickDeriv / drizCR and
written out in include/subpixal_hip.h; parity with drizzlepac is UNPINNED.  ``minmed`` and the other combine types,
``driz_cr_grow``, the CTE tail and static masks are not here.

The per-frame table the kernel reads lives on the device; ``set_map`` and dropping or adding a frame rewrite one
row.  Dropping only clears the frame's ``active`` flag, so the result is bit-identical to a fresh drizzle of the
remaining frames in list order (``output_ctx`` numbers its bits by ``table_names``, dropped frames included).
"""
import numpy as np

from . import _ffi

__all__ = ['DeviceDrizzle', 'KERNELS', 'MAX_FRAMES']

KERNELS = {'square': 0, 'turbo': 1, 'point': 2}            # SPX_DRIZZLE_SQUARE / _TURBO / _POINT
_ROW_MASK = 16                                             # byte offset of a packed row's mask pointer (its third field)
MAX_FRAMES = 128
_DTYPES = ('float32', 'float64')


def _dtype_name(a):
    return str(a.dtype).replace('torch.', '')


def _check_map(m, what):
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
    maps : ``[K, 6]`` forward affine maps, input pixel -> output pixel (0-based, pixel centres on integers).
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
    ``set_config_parameters`` takes the same eight keywords; per-frame values are in the order of ``names``.

    Nothing touches the device before ``execute()``; argument errors are ValueErrors raised here."""

    def __init__(self, frames, maps, out_shape, names=None, weights=None, masks=None, pixfrac=1.0, kernel='square',
                 fill=0.0, cr_reject=False, rms=None, gain=None, sky=None, combine_nlow=0, combine_nhigh=0,
                 driz_cr_snr=(3.5, 3.0), driz_cr_scale=(1.2, 0.7)):
        frames = list(frames)
        K = len(frames)
        if not 1 <= K <= MAX_FRAMES:
            raise ValueError("frames: 1 .. %d frames, got %d." % (MAX_FRAMES, K))
        names = list(range(K)) if names is None else list(names)
        if len(names) != K or len(set(names)) != K:
            raise ValueError("names: one distinct name per frame.")
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
        self._cr = dict(on=False, rms=None, gain=None, sky=None, nlow=0, nhigh=0, snr=(3.5, 3.0), scale=(1.2, 0.7))
        self._rms_dev = {}                             # name -> the resident rms map
        self._crmask, self._merged, self._crclean = {}, {}, {}
        self._fast = False                             # execute() was called by fast_replace_image
        self.set_config_parameters(pixfrac=pixfrac, kernel=kernel, fill=fill, cr_reject=cr_reject, rms=rms, gain=gain,
                                   sky=sky, combine_nlow=combine_nlow, combine_nhigh=combine_nhigh,
                                   driz_cr_snr=driz_cr_snr, driz_cr_scale=driz_cr_scale)
        self._rows_host = None                         # uint8 [K][ROW_BYTES], as spx_drizzle_rows packed them
        self._rows_dev = None
        self._stale = True                             # the whole table must be packed again
        self.output_sci = self.output_wht = self.output_ctx = None
        self.output_median = self.output_nmedian = self.output_crmask = self.output_crclean = None

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
                              sky=None, combine_nlow=None, combine_nhigh=None, driz_cr_snr=None, driz_cr_scale=None):
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
        if cr_reject is not None:
            cr['on'] = bool(cr_reject)
        if cr['on']:
            if cr['rms'] is None:
                raise ValueError("rms: cr_reject needs the frames' noise (a scalar, or per frame a scalar or a map).")
            if min(self._out_shape) < 6:
                raise ValueError("out_shape: cr_reject needs an output of 6 x 6 pixels at least (the blot's quintic).")
        if fill is not None:
            self._fill = fill
        if rms is not None:
            self._rms_dev = {}
        self._cr = cr
        self._stale = True

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

    def crclean(self, name):
        """frame ``name`` with its rejected pixels replaced by the blotted median (the reference's ``crclean_image``),
        or None when the last full ``execute()`` made none"""
        return self._crclean.get(name)

    def map(self, name):
        return self._maps[name].copy()

    def set_map(self, name, affine):
        """Replace the map of frame ``name`` (listed or dropped); one row of the device table is rewritten."""
        if name not in self._maps:
            raise ValueError("set_map: no frame named %r." % (name,))
        old = self._maps[name]
        self._maps[name] = _check_map(affine, repr(name))
        try:
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
        c._maps = {n: m.copy() for n, m in self._maps.items()}
        c._order = list(self._order)
        c._active = dict(self._active)
        c._rows_host = None if self._rows_host is None else self._rows_host.copy()
        c._rows_dev = None if self._rows_dev is None else self._rows_dev.clone()
        c._cr = dict(self._cr)
        c._rms_dev = dict(self._rms_dev)
        # the cosmic-ray masks and the cleaned frames go along (shared tensors, own dicts)
        c._crmask, c._merged, c._crclean = dict(self._crmask), dict(self._merged), dict(self._crclean)
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

    def _pack(self, names, original=False):
        """rows for ``names`` through the library's host entry (ValueError for what it refuses); with cosmic-ray
        rejection on and unless ``original``, a frame's mask is the merged one of the last full ``execute()``"""
        lib = _ffi.load()
        K = len(names)
        fr = [self._resident(n) for n in names]
        frames = np.array([f.data.data_ptr() for f in fr], np.uint64)
        weights = np.array([0 if f.weight is None else f.weight.data_ptr() for f in fr], np.uint64)
        mk = [f.mask if original or not self._cr['on'] or n not in self._merged else self._merged[n]
              for n, f in zip(names, fr)]
        masks = np.array([0 if m is None else m.data_ptr() for m in mk], np.uint64)
        shapes = np.array([tuple(f.data.shape) for f in fr], np.int32)
        maps = np.ascontiguousarray(np.stack([self._maps[n] for n in names]))
        active = np.array([self._active[n] for n in names], np.uint8)
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
        if self._cr['on'] and not self._fast:
            self._reject_cosmic_rays(lib)
        elif not self._cr['on'] and self._merged:
            self._crmask, self._merged, self._crclean = {}, {}, {}
            self._stale = True
        if self._stale or self._rows_dev is None:
            self._rows_host = self._pack(self._order)
            self._rows_dev = torch.from_numpy(self._rows_host).cuda()
            self._stale = False
        dev = self._rows_dev.device
        sci = torch.empty((NY, NX), dtype=torch.float32 if self._dtype == 'float32' else torch.float64, device=dev)
        wht = torch.empty((NY, NX), dtype=torch.float32, device=dev)
        ctx = torch.empty(((K + 31) // 32, NY, NX), dtype=torch.int32, device=dev)
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
        if not active:
            self.output_median = self.output_nmedian = None
            self.output_crmask, self.output_crclean = [], []
            self._stale = True
            return
        host = self._pack(self._order, original=True)
        rows = torch.from_numpy(host).cuda()
        dev, stream = rows.device, device.stream_ptr()
        med = torch.empty((NY, NX), dtype=torch.float32, device=dev)
        nmed = torch.empty((NY, NX), dtype=torch.uint8, device=dev)
        fn = lib.spx_drizzle_median_f32 if f32 else lib.spx_drizzle_median_f64
        _ffi.check(fn(rows.data_ptr(), K, len(active), KERNELS[self._kernel], cr['nlow'], cr['nhigh'], NY, NX,
                      med.data_ptr(), nmed.data_ptr(), stream))
        fn = lib.spx_drizzle_cr_f32 if f32 else lib.spx_drizzle_cr_f64
        host = host.copy()
        for name in active:
            f = self._pool[name]
            ny, nx = f.data.shape
            rs, rm = self._rms_of(name)
            gain = None if cr['gain'] is None else cr['gain'][name]
            sky = 0.0 if cr['sky'] is None else cr['sky'][name]
            mask = torch.empty((ny, nx), dtype=torch.uint8, device=dev)
            clean = torch.empty_like(f.data)
            _ffi.check(fn(rows.data_ptr(), K, self._order.index(name), ny, nx, med.data_ptr(), nmed.data_ptr(), NY, NX,
                          rs, None if rm is None else rm.data_ptr(), sky, float('nan') if gain is None else gain,
                          cr['snr'][0], cr['snr'][1], cr['scale'][0], cr['scale'][1], mask.data_ptr(),
                          clean.data_ptr(), stream))
            self._crmask[name], self._crclean[name] = mask, clean
            self._merged[name] = mask if f.mask is None else (f.mask | mask)
            host[self._order.index(name), _ROW_MASK:_ROW_MASK + 8].view(np.uint64)[0] = self._merged[name].data_ptr()
        self.output_median, self.output_nmedian = med, nmed
        self.output_crmask = [self._crmask[n] for n in active]
        self.output_crclean = [self._crclean[n] for n in active]
        self._rows_host, self._rows_dev = host, torch.from_numpy(host).cuda()
        self._stale = False
