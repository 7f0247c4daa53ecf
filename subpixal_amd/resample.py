"""Drizzle of dithered frames on the device, with the leave-one-out interface of the reference's ``Resample``
(subpixal/resample.py) where that has a meaning without files, WCS objects and drizzlepac.

``DeviceDrizzle`` holds K frames (CUDA tensors), one forward affine map per frame -- input pixel -> output pixel,
``(X, Y) = (a0 x + a1 y + a2, a3 x + a4 y + a5)``, the ``[6]`` layout of ``blot.shift_affine`` -- and a fixed output
grid.  ``execute()`` is one launch of the gather kernel of csrc/spx_drizzle_kernels.h (``spx_drizzle_f32`` /
``_f64``); include/subpixal_hip.h carries the definition in full.  ``output_sci`` is the weighted MEAN of the input
values that land on a pixel, i.e. input-pixel surface brightness: no ``scale**2`` is applied when the map changes the
pixel area.  drizzlepac is not in the reference tree, so parity with it is UNPINNED (the definition is this
library's own, after Fruchter & Hook 2002); polynomial distortion, cosmic-ray rejection, the median step, sky
subtraction and FITS input/output are not here.

The per-frame table the kernel reads lives on the device; ``set_map`` and dropping or adding a frame rewrite one
row.  Dropping only clears the frame's ``active`` flag, so the result is bit-identical to a fresh drizzle of the
remaining frames in list order (``output_ctx`` numbers its bits by ``table_names``, dropped frames included).
"""
import numpy as np

from . import _ffi

__all__ = ['DeviceDrizzle', 'KERNELS', 'MAX_FRAMES']

KERNELS = {'square': 0, 'turbo': 1, 'point': 2}            # SPX_DRIZZLE_SQUARE / _TURBO / _POINT
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

    Nothing touches the device before ``execute()``; argument errors are ValueErrors raised here."""

    def __init__(self, frames, maps, out_shape, names=None, weights=None, masks=None, pixfrac=1.0, kernel='square',
                 fill=0.0):
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
        self.set_config_parameters(pixfrac=pixfrac, kernel=kernel, fill=fill)
        self._rows_host = None                         # uint8 [K][ROW_BYTES], as spx_drizzle_rows packed them
        self._rows_dev = None
        self._stale = True                             # the whole table must be packed again
        self.output_sci = self.output_wht = self.output_ctx = None
        self.output_crclean = None

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

    def set_config_parameters(self, pixfrac=None, kernel=None, fill=None):
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
            self._fill = float(fill)
        self._stale = True

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
        self.execute()

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

    def _pack(self, names):
        """rows for ``names`` through the library's host entry (ValueError for what it refuses)"""
        lib = _ffi.load()
        K = len(names)
        fr = [self._resident(n) for n in names]
        frames = np.array([f.data.data_ptr() for f in fr], np.uint64)
        weights = np.array([0 if f.weight is None else f.weight.data_ptr() for f in fr], np.uint64)
        masks = np.array([0 if f.mask is None else f.mask.data_ptr() for f in fr], np.uint64)
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
        (int32 ``[ceil(K / 32), NY, NX]``, K = ``len(table_names)``) are new CUDA tensors after every call."""
        import torch
        from . import device
        device.init()
        lib = _ffi.load()
        K = len(self._order)
        if self._stale or self._rows_dev is None:
            self._rows_host = self._pack(self._order)
            self._rows_dev = torch.from_numpy(self._rows_host).cuda()
            self._stale = False
        NY, NX = self._out_shape
        dev = self._rows_dev.device
        sci = torch.empty((NY, NX), dtype=torch.float32 if self._dtype == 'float32' else torch.float64, device=dev)
        wht = torch.empty((NY, NX), dtype=torch.float32, device=dev)
        ctx = torch.empty(((K + 31) // 32, NY, NX), dtype=torch.int32, device=dev)
        fn = lib.spx_drizzle_f32 if self._dtype == 'float32' else lib.spx_drizzle_f64
        _ffi.check(fn(self._rows_dev.data_ptr(), K, KERNELS[self._kernel], self._fill, NY, NX, sci.data_ptr(),
                      wht.data_ptr(), ctx.data_ptr(), device.stream_ptr()))
        self.output_sci, self.output_wht, self.output_ctx = sci, wht, ctx
        return self
