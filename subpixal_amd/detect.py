"""Source finding on the device: detection threshold -> connected-component labelling -> isophotal
measurements -> the ``cutout.CutoutCatalog`` that ``align.find_linear_fit`` takes.

The reference gets its segmentation image and source positions from SExtractor, an external program
(``catalogs.py``: ``SExImageCatalog``); this module is the device-resident stand-in for that step.  Its
definitions are its own (``include/subpixal_hip.h``, ``csrc/spx_detect_kernels.h``): parity with SExtractor is
unpinned.  Merged sources are split on request (:func:`deblend`, ``find_sources(..., deblend=True)``: a
multi-threshold tree and a flood per segment, ``csrc/spx_deblend_kernels.h``).  With a noise map the sources also
get a flux error, a FWHM and from them the reference's ``pos_std`` and fit ``weight`` (:func:`measure_errors`,
``find_sources(..., rms=...)``, ``detect_sources(..., errors=True)``: ``csrc/spx_error_kernels.h``); the
catalogue filter language lives in :mod:`subpixal_amd.catalogs`.

The two inputs of detection that matter, the threshold and the background, come from the frame itself:
:func:`estimate_background` builds the sky and noise maps on the device (sigma-clipped statistics on a mesh of
cells, median filter, bicubic spline: ``csrc/spx_background_kernels.h``), and :func:`detect_sources` chains it
with :func:`find_sources`::

    src = detect.detect_sources(frame, nsigma=1.5, box=(64, 64), min_area=5)
    src.background_model.background, src.background_model.rms      # CUDA tensors, the frame's shape and dtype
"""
import numpy as np
import torch

from . import _ffi, cutout, device

COLUMNS = ('npix', 'flux', 'x', 'y', 'x2', 'y2', 'xy', 'a', 'b', 'theta', 'peak', 'xpeak', 'ypeak')
FLAG_BORDER, FLAG_NOFLUX, FLAG_BADPIX = 1, 2, 4
FLAG_DEBLENDED, FLAG_NODEBLEND = 8, 16       # a child of a split parent; a parent over the box limit, not examined
FLAG_HALFMAX, FLAG_NOISE = 32, 64             # every usable pixel above half maximum (fwhm is a lower bound); bad rms
ERROR_COLUMNS = ('fluxerr', 'errx2', 'erry2', 'errxy', 'nhalf', 'fwhm')
FWHM2SIGMA = 2.0 * np.sqrt(2.0 * np.log(2.0))         # the reference's _FWHM2SIGMA (catalogs.py:31)
DEBLEND_MODES = {'exponential': 0, 'linear': 1}
MAX_FILTER_SIDE = 7
MIN_BOX, MAX_BOX = 8, 128                    # background mesh cells: sides, and pixels per cell by dtype
MAX_CELL_PIXELS = {False: 16384, True: 8192}


def _is_f64(frame):
    if isinstance(frame, torch.Tensor):
        return frame.dtype == torch.float64
    return np.asarray(frame).dtype == np.float64


def _frame_or_scalar(v, shape, tdt, name):
    """(scalar, None) or (0.0, CUDA tensor of `tdt` and the frame's shape)"""
    if isinstance(v, torch.Tensor) or np.ndim(v) > 0:
        if tuple(np.shape(v)) != tuple(shape):
            raise ValueError("%s must be a scalar or have the shape of the frame." % name)
        return 0.0, device.to_device(v, tdt)
    return float(v), None


def _check_arguments(frame, mask, filter_kernel, min_area, connectivity):
    """Everything that can be refused without touching the device."""
    if frame.ndim != 2:
        raise ValueError("frame must be 2-D.")
    if frame.shape[0] < 1 or frame.shape[1] < 1 or frame.shape[0] * frame.shape[1] >= 2 ** 31 - 1:
        raise ValueError("frame must hold between 1 and 2**31 - 2 pixels.")
    if connectivity not in (4, 8):
        raise ValueError("connectivity must be 4 or 8.")
    if int(min_area) != min_area or min_area < 1:
        raise ValueError("min_area must be an integer >= 1.")
    if mask is not None and tuple(np.shape(mask)) != tuple(frame.shape):
        raise ValueError("mask must have the shape of the frame.")
    if filter_kernel is not None:
        k = filter_kernel
        if k.ndim != 2 or k.shape[0] % 2 == 0 or k.shape[1] % 2 == 0:
            raise ValueError("filter_kernel must be 2-D with odd sides.")
        if max(k.shape) > MAX_FILTER_SIDE:
            raise ValueError("filter_kernel sides must be at most %d." % MAX_FILTER_SIDE)


def _check_deblend_arguments(levels, contrast, mode):
    if int(levels) != levels or levels + 1 not in (2, 4, 8, 16, 32, 64):
        raise ValueError("deblending levels must be 1, 3, 7, 15, 31 or 63 (levels + 1 a power of two).")
    if not 0.0 <= contrast <= 1.0:
        raise ValueError("deblending contrast must lie in 0..1.")
    if mode not in DEBLEND_MODES:
        raise ValueError("deblending mode must be 'exponential' or 'linear'.")


class Sources(object):
    """What :func:`find_sources` found.  ``segmentation``: int32 CUDA tensor ``[ny, nx]`` with labels
    ``1..len(self)`` in raster order of each segment's first pixel.  Per source (numpy, index = label - 1):
    ``id``, ``x``, ``y`` (0-based pixel centres, the convention of ``CutoutCatalog.src_pos``), ``flux``,
    ``npix``, central moments ``x2, y2, xy``, ellipse ``a, b, theta`` (degrees), ``peak`` at ``xpeak, ypeak``,
    ``flags`` (``FLAG_BORDER | FLAG_NOFLUX | FLAG_BADPIX``, with deblending also ``FLAG_DEBLENDED |
    FLAG_NODEBLEND``) and ``bbox`` = (xmin, ymin, xmax, ymax) inclusive.  ``parent``: with deblending, the number
    the source's segment had BEFORE deblending (children of one merged detection share it), else ``None``.
    ``table_device`` / ``flags_device`` are the same numbers as CUDA tensors.

    When errors were measured (``find_sources(..., rms=...)``; ``has_errors``): ``fluxerr``, the centre's
    covariance ``errx2, erry2, errxy``, ``nhalf`` and ``fwhm`` from :func:`measure_errors` (``errors_device`` is the
    CUDA tensor), and on the host ``snr = flux / fluxerr``, ``pos_std = fwhm / (2 sqrt(2 ln 2) snr)`` and ``weight =
    1 / pos_std**2`` by the reference's formulas (catalogs.py:405-428, 968-987); ``flags`` then also carries
    ``FLAG_HALFMAX | FLAG_NOISE``.  Without them none of these attributes exists."""
    has_errors = False

    def __init__(self, segmentation, table, flags, bbox, parent=None, errors=None):
        self.segmentation = segmentation
        self.parent = None if parent is None else parent.cpu().numpy()
        self.table_device, self.flags_device = table, flags
        t = table.cpu().numpy()
        for i, c in enumerate(COLUMNS):
            setattr(self, c, t[:, i].astype(np.int32) if c in ('npix', 'xpeak', 'ypeak') else t[:, i].copy())
        self.flags = flags.cpu().numpy()
        self.bbox = bbox.cpu().numpy()
        self.id = np.arange(1, len(self.flags) + 1, dtype=np.int32)
        if errors is not None:
            self.has_errors = True
            self.errors_device = errors
            e = errors.cpu().numpy()
            for i, c in enumerate(ERROR_COLUMNS):
                setattr(self, c, e[:, i].astype(np.int32) if c == 'nhalf' else e[:, i].copy())
            with np.errstate(all='ignore'):
                self.snr = self.flux / self.fluxerr
                self.pos_std = position_std(self.fwhm, self.flux, self.fluxerr)
                self.weight = 1.0 / self.pos_std ** 2

    def __len__(self):
        return len(self.id)

    def table(self):
        """Columns under the names the reference's catalogs use (catalogs.py:75-93) where it has one."""
        out = {'id': self.id, 'x': self.x, 'y': self.y, 'flux': self.flux, 'semi-major-a': self.a,
               'semi-major-b': self.b}
        for c in ('npix', 'x2', 'y2', 'xy', 'theta', 'peak', 'xpeak', 'ypeak', 'flags'):
            out[c] = getattr(self, c)
        if self.parent is not None:
            out['parent'] = self.parent
        if self.has_errors:
            for c in ERROR_COLUMNS + ('snr', 'pos_std', 'weight'):
                out[c] = getattr(self, c)
        return out

    def cutout_catalog(self, frame, pad=1, dtype=np.float32, weight=None, mask=None):
        """The primary cutouts of ``frame`` as a :class:`cutout.CutoutCatalog`, by the reference's rules
        (``cutout.primary_cutout_boxes``: segments touching the border are skipped, box = bounding rectangle +
        ``pad``), with ``src_pos = (x, y)``, ``src_id`` and this segmentation.  ``weight=None``: no source weights
        (what the reference's ``compute_weights`` amounts to for equal weights); ``weight='flux'``: the fluxes;
        ``weight='pos_std'``: the ``weight`` column, ``1 / pos_std**2`` (what ``SExImageCatalog.compute_weights``
        gives; needs measured errors).  Sources without a position (``FLAG_NOFLUX``) are left out, and with
        ``weight='pos_std'`` so are sources whose weight is not finite or not positive."""
        return self._cutout_catalog(frame, pad, dtype, weight, mask, None)

    def _cutout_catalog(self, frame, pad, dtype, weight, mask, select):
        if weight not in (None, 'flux', 'pos_std'):
            raise ValueError("weight must be None, 'flux' or 'pos_std'.")
        if weight == 'pos_std' and not self.has_errors:
            raise ValueError("weight='pos_std' needs measured errors: find_sources(..., rms=...) or "
                             "detect_sources(..., errors=True).")
        ids, boxes = cutout.primary_cutout_boxes(self.segmentation, pad=pad)
        keep = (self.flags[ids - 1] & FLAG_NOFLUX) == 0
        if weight == 'pos_std':
            wt = self.weight[ids - 1]
            keep &= np.isfinite(wt) & (wt > 0)
        if select is not None:
            keep &= np.isin(ids, select)
        ids, boxes = ids[keep], boxes[keep]
        k = ids - 1
        src_weight = None if weight is None else (self.flux[k] if weight == 'flux' else self.weight[k])
        return cutout.CutoutCatalog(frame, boxes, src_pos=np.stack([self.x[k], self.y[k]], axis=1),
                                    src_weight=src_weight, src_id=ids, mask=mask,
                                    segmentation_image=self.segmentation, dtype=dtype)


def position_std(fwhm, flux, fluxerr):
    """The reference's position error estimate (catalogs.py:405-428): ``fwhm / (2 sqrt(2 ln 2) * flux / fluxerr)``,
    written with its operations in its order."""
    with np.errstate(all='ignore'):
        return np.asarray(fwhm / (FWHM2SIGMA * flux / fluxerr))


def label(frame, threshold, mask=None, filter_kernel=None, min_area=5, connectivity=8):
    """Segmentation image only: ``(labels int32 CUDA [ny, nx], nlabels)`` (``spx_detect_label_f32/_f64``).
    Arguments as :func:`find_sources`."""
    fshape = frame if isinstance(frame, torch.Tensor) else np.asarray(frame)
    kern = None if filter_kernel is None else np.asarray(filter_kernel)
    _check_arguments(fshape, mask, kern, min_area, connectivity)
    f64 = _is_f64(frame)
    tdt = torch.float64 if f64 else torch.float32
    f = device.to_device(frame, tdt)
    thr, thr_map = _frame_or_scalar(threshold, f.shape, torch.float32, 'threshold')
    m = None if mask is None else device.to_device(mask, torch.uint8)
    k = None if kern is None else device.to_device(kern, tdt)
    fky, fkx = (1, 1) if kern is None else kern.shape
    ny, nx = f.shape
    lib = _ffi.load()
    nbytes = lib.spx_detect_workspace_bytes(ny, nx)
    work = torch.empty((nbytes,), dtype=torch.uint8, device=f.device)
    labels = torch.empty((ny, nx), dtype=torch.int32, device=f.device)
    nlab = torch.empty((1,), dtype=torch.int32, device=f.device)
    fn = lib.spx_detect_label_f64 if f64 else lib.spx_detect_label_f32
    with torch.cuda.device(f.device):
        _ffi.check(fn(device.ptr(f), device.ptr(m), thr, device.ptr(thr_map), device.ptr(k), int(fky), int(fkx),
                      ny, nx, int(connectivity), int(min_area), device.ptr(work), nbytes, device.ptr(labels),
                      device.ptr(nlab), device.stream_ptr()))
    n = int(nlab.item())
    if n < 0:
        raise _ffi.SubpixalHipError("component merge failed its consistency check (spx_detect_label).")
    return labels, n


def measure(frame, labels, nlabels, background=0.0, mask=None, _all_boxes=False):
    """Isophotal measurements of labels ``1..nlabels`` (``spx_label_bboxes_i32`` + ``spx_measure_labels_f32/_f64``).
    Returns CUDA tensors ``(table float64 [nlabels, 13] in COLUMNS order, flags int32 [nlabels], bbox int32
    [nlabels, 4])``."""
    f64 = _is_f64(frame)
    tdt = torch.float64 if f64 else torch.float32
    f = device.to_device(frame, tdt)
    seg = device.to_device(labels, torch.int32)
    if f.dim() != 2 or tuple(seg.shape) != tuple(f.shape):
        raise ValueError("frame must be 2-D and labels must have its shape.")
    if mask is not None and tuple(np.shape(mask)) != tuple(f.shape):
        raise ValueError("mask must have the shape of the frame.")
    bkg, bkg_map = _frame_or_scalar(background, f.shape, tdt, 'background')
    m = None if mask is None else device.to_device(mask, torch.uint8)
    boxes, _ = cutout.segment_bounding_boxes(seg, max_label=nlabels)
    table = torch.empty((nlabels, len(COLUMNS)), dtype=torch.float64, device=f.device)
    flags = torch.empty((nlabels,), dtype=torch.int32, device=f.device)
    lib = _ffi.load()
    fn = lib.spx_measure_labels_f64 if f64 else lib.spx_measure_labels_f32
    with torch.cuda.device(f.device):
        _ffi.check(fn(device.ptr(f), device.ptr(m), bkg, device.ptr(bkg_map), device.ptr(seg), f.shape[0],
                      f.shape[1], int(nlabels), device.ptr(boxes), device.ptr(table), device.ptr(flags),
                      device.stream_ptr()))
    return table, flags, (boxes if _all_boxes else boxes[1:])          # (_all_boxes: with row 0, as the C entries take it)


def _check_error_arguments(rms, gain, shape):
    if rms is None:
        raise ValueError("rms must be a scalar or a frame, not None.")
    if (isinstance(rms, torch.Tensor) or np.ndim(rms) > 0) and tuple(np.shape(rms)) != tuple(shape):
        raise ValueError("rms must be a scalar or have the shape of the frame.")
    if gain is not None and not (np.ndim(gain) == 0 and float(gain) > 0 and np.isfinite(float(gain))):
        raise ValueError("gain must be None or a positive, finite scalar.")


def measure_errors(frame, labels, nlabels, table, rms, background=0.0, gain=None, mask=None, _boxes=None):
    """Error measurements of labels ``1..nlabels`` (``spx_label_bboxes_i32`` + ``spx_measure_errors_f32/_f64``; the
    definitions are in ``include/subpixal_hip.h``).

    frame, labels, nlabels, background, mask : as given to :func:`measure`.
    table : the table :func:`measure` returned for them (flux, x, y and peak are taken from it).
    rms : the noise per pixel, a scalar or a frame (used in the frame's dtype): ``Background.rms``.
    gain : electrons per data unit; adds the source's own Poisson noise ``w / gain`` where ``w > 0``.  None: none.

    Returns CUDA tensors ``(errors float64 [nlabels, 6] in ERROR_COLUMNS order, eflags int32 [nlabels])`` with
    ``FLAG_HALFMAX`` / ``FLAG_NOISE``.  Bit-identical from run to run."""
    shape = tuple(np.shape(frame))
    if len(shape) != 2 or tuple(np.shape(labels)) != shape:
        raise ValueError("frame must be 2-D and labels must have its shape.")
    if mask is not None and tuple(np.shape(mask)) != shape:
        raise ValueError("mask must have the shape of the frame.")
    if int(nlabels) != nlabels or nlabels < 0:
        raise ValueError("nlabels must be an integer >= 0.")
    nlabels = int(nlabels)
    _check_error_arguments(rms, gain, shape)
    if np.ndim(background) > 0 and tuple(np.shape(background)) != shape:
        raise ValueError("background must be a scalar or have the shape of the frame.")
    if tuple(np.shape(table)) != (nlabels, len(COLUMNS)):
        raise ValueError("table must be the [nlabels, %d] table of measure()." % len(COLUMNS))
    f64 = _is_f64(frame)
    tdt = torch.float64 if f64 else torch.float32
    f = device.to_device(frame, tdt)
    seg = device.to_device(labels, torch.int32)
    bkg, bkg_map = _frame_or_scalar(background, f.shape, tdt, 'background')
    sig, sig_map = _frame_or_scalar(rms, f.shape, tdt, 'rms')
    m = None if mask is None else device.to_device(mask, torch.uint8)
    tab = device.to_device(table, torch.float64)
    boxes = _boxes                                   # (find_sources hands over the table measure() made)
    if boxes is None:
        boxes, _ = cutout.segment_bounding_boxes(seg, max_label=nlabels)
    errors = torch.empty((nlabels, len(ERROR_COLUMNS)), dtype=torch.float64, device=f.device)
    eflags = torch.empty((nlabels,), dtype=torch.int32, device=f.device)
    lib = _ffi.load()
    fn = lib.spx_measure_errors_f64 if f64 else lib.spx_measure_errors_f32
    with torch.cuda.device(f.device):
        _ffi.check(fn(device.ptr(f), device.ptr(m), bkg, device.ptr(bkg_map), sig, device.ptr(sig_map),
                      0.0 if gain is None else float(gain), device.ptr(seg), f.shape[0], f.shape[1], nlabels,
                      device.ptr(boxes), device.ptr(tab), device.ptr(errors), device.ptr(eflags),
                      device.stream_ptr()))
    return errors, eflags


def deblend(frame, labels, nlabels, mask=None, filter_kernel=None, levels=31, contrast=0.005, mode='exponential',
            min_area=5, connectivity=8):
    """Split the merged sources of a label image (``spx_label_bboxes_i32`` + ``spx_deblend_labels_f32/_f64``; the
    definition is in ``include/subpixal_hip.h``): per segment, a tree of its connected components above ``levels``
    thresholds between its faintest and brightest (filtered) pixel, spaced exponentially or linearly; a branch
    counts when it holds at least ``contrast`` of the segment's quantised flux and ``min_area`` pixels; a segment
    with two or more such branches is divided among them by a flood that descends level by level.

    frame, mask, filter_kernel, min_area, connectivity : as given to :func:`label` for ``labels``.
    labels, nlabels : the segmentation (int32, labels ``1..nlabels``).

    Returns CUDA tensors ``(labels int32 [ny, nx], nlabels, parent int32 [nlabels], dflags int32 [nlabels])``:
    every final segment numbered in raster order of its first pixel, the input label it came from, and
    ``FLAG_DEBLENDED`` / ``FLAG_NODEBLEND`` (a box of more than 65536 pixels is not examined).  Bit-identical
    from run to run.

    Memory: every call allocates its scratch anew, ``spx_deblend_workspace_bytes(ny, nx, nlabels)`` bytes: 8 bytes
    per frame pixel for the numbering, plus ``min(nlabels, 64)`` slots of 36 bytes per pixel of the largest box a
    parent may have (``min(65536, ny * nx)``) for the parents that do not fit LDS -- about 150 MB for any frame of
    65536 pixels or more with 64 labels or more, whether or not a parent comes near that size."""
    fshape = frame if isinstance(frame, torch.Tensor) else np.asarray(frame)
    kern = None if filter_kernel is None else np.asarray(filter_kernel)
    _check_arguments(fshape, mask, kern, min_area, connectivity)
    _check_deblend_arguments(levels, contrast, mode)
    if tuple(np.shape(labels)) != tuple(fshape.shape):
        raise ValueError("labels must have the shape of the frame.")
    if int(nlabels) != nlabels or nlabels < 0:
        raise ValueError("nlabels must be an integer >= 0.")
    f64 = _is_f64(frame)
    tdt = torch.float64 if f64 else torch.float32
    f = device.to_device(frame, tdt)
    seg = device.to_device(labels, torch.int32)
    m = None if mask is None else device.to_device(mask, torch.uint8)
    k = None if kern is None else device.to_device(kern, tdt)
    fky, fkx = (1, 1) if kern is None else kern.shape
    ny, nx = f.shape
    nlabels = int(nlabels)
    boxes, _ = cutout.segment_bounding_boxes(seg, max_label=nlabels)
    lib = _ffi.load()
    nbytes = lib.spx_deblend_workspace_bytes(ny, nx, nlabels)
    work = torch.empty((nbytes,), dtype=torch.uint8, device=f.device)
    out = torch.empty((ny, nx), dtype=torch.int32, device=f.device)
    nout = torch.empty((1,), dtype=torch.int32, device=f.device)
    fn = lib.spx_deblend_labels_f64 if f64 else lib.spx_deblend_labels_f32
    max_out = min(ny * nx, 2 * nlabels + 1024)       # a guess; the call reports the true count, so a miss is seen
    while True:
        table = torch.empty((2, max_out), dtype=torch.int32, device=f.device)
        with torch.cuda.device(f.device):
            _ffi.check(fn(device.ptr(f), device.ptr(m), device.ptr(k), int(fky), int(fkx), ny, nx, device.ptr(seg),
                          nlabels, device.ptr(boxes), int(connectivity), int(min_area), int(levels), float(contrast),
                          DEBLEND_MODES[mode], device.ptr(work), nbytes, device.ptr(out), device.ptr(table[0]),
                          device.ptr(table[1]), max_out, device.ptr(nout), device.stream_ptr()))
        n = int(nout.item())
        if n <= max_out:
            break
        max_out = n                                  # rows beyond max_out were not written: once more, with room
    if n < 0:
        raise _ffi.SubpixalHipError("component merge failed its consistency check (spx_deblend_labels).")
    return out, n, table[0, :n], table[1, :n]


_deblend = deblend           # find_sources has a keyword of the same name


def find_sources(frame, threshold, background=0.0, mask=None, filter_kernel=None, min_area=5, connectivity=8,
                 deblend=False, deblend_levels=31, deblend_contrast=0.005, deblend_mode='exponential', rms=None,
                 gain=None):
    """Detect, label and measure the sources of ``frame`` on the device.

    frame : 2-D numpy array or CUDA tensor; float64 frames are processed in float64, everything else in float32.
    threshold : scalar, or a per-pixel frame (used as float32).  A pixel is detected when it is finite, not
        masked and its (filtered) value is ``> threshold``.
    background : scalar or per-pixel frame subtracted for the MEASUREMENTS (which use the unfiltered frame);
        detection compares against ``threshold`` alone.
    mask : booleans ``[ny, nx]``, True = bad, or None.
    filter_kernel : 2-D weights with odd sides <= 7 the frame is correlated with before thresholding, used as
        given (normalise them yourself); pixels outside the frame, masked or non-finite count as 0 and the
        weights are not renormalised there.
    min_area : components with fewer pixels are dropped.  connectivity : 8 or 4.

    deblend : split merged sources (:func:`deblend` with ``deblend_levels``, ``deblend_contrast``,
        ``deblend_mode``) between labelling and measuring: the measurements are those of the deblended segments,
        ``Sources.parent`` holds each one's segment number before deblending and ``flags`` gains
        ``FLAG_DEBLENDED`` / ``FLAG_NODEBLEND``.  Off by default; nothing changes then.

    rms : the noise per pixel, a scalar or a frame (``Background.rms``).  Given, the sources are also measured by
        :func:`measure_errors` (with ``gain``, electrons per data unit, for the sources' own Poisson noise):
        :class:`Sources` gains ``fluxerr, errx2, erry2, errxy, nhalf, fwhm, snr, pos_std, weight`` and ``flags`` gains
        ``FLAG_HALFMAX`` / ``FLAG_NOISE``.  None (the default): nothing changes.

    Returns a :class:`Sources`.  Labels are numbered in raster order of each component's first pixel, as
    ``scipy.ndimage.label`` numbers them; all results are bit-identical from run to run."""
    _check_arguments(frame if isinstance(frame, torch.Tensor) else np.asarray(frame), mask,
                     None if filter_kernel is None else np.asarray(filter_kernel), min_area, connectivity)
    if deblend:
        _check_deblend_arguments(deblend_levels, deblend_contrast, deblend_mode)
    if rms is not None:
        _check_error_arguments(rms, gain, np.shape(frame))
    elif gain is not None:
        raise ValueError("gain needs rms: errors are measured only with a noise map.")
    frame = device.to_device(frame, torch.float64 if _is_f64(frame) else torch.float32)     # one upload for both steps
    mask = None if mask is None else device.to_device(mask, torch.uint8)
    labels, n = label(frame, threshold, mask=mask, filter_kernel=filter_kernel, min_area=min_area,
                      connectivity=connectivity)
    parent = None
    if not deblend:
        table, flags, boxes = measure(frame, labels, n, background=background, mask=mask, _all_boxes=True)
        if rms is None:
            return Sources(labels, table, flags, boxes[1:])
    else:
        labels, n, parent, dflags = _deblend(frame, labels, n, mask=mask, filter_kernel=filter_kernel,
                                             levels=deblend_levels, contrast=deblend_contrast, mode=deblend_mode,
                                             min_area=min_area, connectivity=connectivity)
        table, flags, boxes = measure(frame, labels, n, background=background, mask=mask, _all_boxes=True)
        flags = flags | dflags
        if rms is None:
            return Sources(labels, table, flags, boxes[1:], parent=parent)
    errors, eflags = measure_errors(frame, labels, n, table, rms, background=background, gain=gain, mask=mask,
                                    _boxes=boxes)
    return Sources(labels, table, flags | eflags, boxes[1:], parent=parent, errors=errors)


def _check_background_arguments(frame, box, filter_size, mask, exclude, sigma, max_iters, min_good_fraction, f64):
    """Everything :func:`estimate_background` can refuse without touching the device."""
    if frame.ndim != 2:
        raise ValueError("frame must be 2-D.")
    if frame.shape[0] < 1 or frame.shape[1] < 1 or frame.shape[0] * frame.shape[1] >= 2 ** 31 - 1:
        raise ValueError("frame must hold between 1 and 2**31 - 2 pixels.")
    try:
        bh, bw = box
        ok = int(bh) == bh and int(bw) == bw
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("box must be a pair of integers (height, width).")
    if not (MIN_BOX <= bh <= MAX_BOX and MIN_BOX <= bw <= MAX_BOX):
        raise ValueError("box sides must lie in %d..%d." % (MIN_BOX, MAX_BOX))
    if bh * bw > MAX_CELL_PIXELS[f64]:
        raise ValueError("box must hold at most %d pixels for %s frames."
                         % (MAX_CELL_PIXELS[f64], 'float64' if f64 else 'float32'))
    if filter_size not in (1, 3, 5, 7):
        raise ValueError("filter_size must be 1, 3, 5 or 7.")
    if mask is not None and tuple(np.shape(mask)) != tuple(frame.shape):
        raise ValueError("mask must have the shape of the frame.")
    if exclude is not None:
        if tuple(np.shape(exclude)) != tuple(frame.shape):
            raise ValueError("exclude must have the shape of the frame.")
        if exclude.dtype != (torch.int32 if isinstance(exclude, torch.Tensor) else np.dtype(np.int32)):
            raise ValueError("exclude must be an int32 label image.")
    if not (sigma > 0 and np.isfinite(sigma)):
        raise ValueError("sigma must be positive and finite.")
    if int(max_iters) != max_iters or max_iters < 0:
        raise ValueError("max_iters must be an integer >= 0.")
    if not 0.0 <= min_good_fraction <= 1.0:
        raise ValueError("min_good_fraction must lie in 0..1.")


class Background(object):
    """What :func:`estimate_background` built.  ``background``, ``rms``: CUDA tensors of the frame's shape and
    dtype.  On the mesh ``[ncy, ncx]`` (numpy): ``mesh_background``, ``mesh_rms`` AFTER the median filter (the
    nodes the spline goes through); ``mesh_background_raw``, ``mesh_rms_raw`` BEFORE it (NaN in bad cells) and
    ``mesh_ngood``, the usable pixels per cell before clipping.  ``box``, ``filter_size`` as given."""

    def __init__(self, frame_shape, f64, box, filter_size, mesh, work, background, rms, thresholds):
        self.box, self.filter_size = box, filter_size
        self._shape, self._f64, self._mesh, self._work = frame_shape, f64, mesh, work
        self.background, self.rms = background, rms
        self._thr = thresholds
        ncy, ncx = mesh[2].shape
        nc = ncy * ncx
        planes = work[:2 * 6 * nc * 8].view(torch.float64).view(2, 6, ncy, ncx)
        self.mesh_background = planes[0, 0].cpu().numpy()
        self.mesh_rms = planes[1, 0].cpu().numpy()
        self.mesh_background_raw = mesh[0].cpu().numpy()
        self.mesh_rms_raw = mesh[1].cpu().numpy()
        self.mesh_ngood = mesh[2].cpu().numpy()

    def threshold(self, nsigma):
        """float32 CUDA tensor ``background + nsigma * rms`` (from the maps as stored), the threshold frame
        :func:`find_sources` takes.  Evaluated on the device, once per ``nsigma``."""
        nsigma = float(nsigma)
        if nsigma not in self._thr:
            thr = torch.empty(self._shape, dtype=torch.float32, device=self.background.device)
            _background_maps(self._mesh, self.box, self.filter_size, self._shape, self._f64, self._work, nsigma,
                             None, None, thr)
            self._thr = {nsigma: thr}
        return self._thr[nsigma]


def _background_maps(mesh, box, filter_size, shape, f64, work, nsigma, bkg, rms, thr):
    lib = _ffi.load()
    ncy, ncx = mesh[2].shape
    status = torch.empty((1,), dtype=torch.int32, device=work.device)
    fn = lib.spx_background_maps_f64 if f64 else lib.spx_background_maps_f32
    with torch.cuda.device(work.device):
        _ffi.check(fn(device.ptr(mesh[0]), device.ptr(mesh[1]), device.ptr(mesh[2]), ncy, ncx, int(box[0]), int(box[1]),
                      int(filter_size), int(shape[0]), int(shape[1]), float(nsigma), device.ptr(work), work.numel(),
                      device.ptr(bkg), device.ptr(rms), device.ptr(thr), device.ptr(status), device.stream_ptr()))
    if int(status.item()) & 1:
        raise _ffi.SubpixalHipError("the background mesh has no good cell (too few usable pixels in every cell).")


def _estimate_background(frame, box, filter_size, mask, exclude, sigma, max_iters, min_good_fraction, nsigma=None):
    fshape = frame if isinstance(frame, torch.Tensor) else np.asarray(frame)
    f64 = _is_f64(frame)
    ex = exclude if exclude is None or isinstance(exclude, torch.Tensor) else np.asarray(exclude)
    _check_background_arguments(fshape, box, filter_size, mask, ex, sigma, max_iters, min_good_fraction, f64)
    tdt = torch.float64 if f64 else torch.float32
    f = device.to_device(frame, tdt)
    m = None if mask is None else device.to_device(mask, torch.uint8)
    lab = None if ex is None else device.to_device(ex, torch.int32)
    ny, nx = f.shape
    bh, bw = int(box[0]), int(box[1])
    ncy, ncx = -(-ny // bh), -(-nx // bw)
    lib = _ffi.load()
    mesh = (torch.empty((ncy, ncx), dtype=torch.float64, device=f.device),
            torch.empty((ncy, ncx), dtype=torch.float64, device=f.device),
            torch.empty((ncy, ncx), dtype=torch.int32, device=f.device))
    fn = lib.spx_background_mesh_f64 if f64 else lib.spx_background_mesh_f32
    with torch.cuda.device(f.device):
        _ffi.check(fn(device.ptr(f), device.ptr(m), device.ptr(lab), ny, nx, bh, bw, float(sigma), int(max_iters),
                      float(min_good_fraction), device.ptr(mesh[0]), device.ptr(mesh[1]), device.ptr(mesh[2]),
                      device.stream_ptr()))
    work = torch.empty((lib.spx_background_workspace_bytes(ny, nx, bh, bw),), dtype=torch.uint8, device=f.device)
    bkg = torch.empty((ny, nx), dtype=tdt, device=f.device)
    rms = torch.empty((ny, nx), dtype=tdt, device=f.device)
    thr = None if nsigma is None else torch.empty((ny, nx), dtype=torch.float32, device=f.device)
    _background_maps(mesh, (bh, bw), filter_size, (ny, nx), f64, work, 0.0 if nsigma is None else nsigma, bkg, rms,
                     thr)
    return Background((ny, nx), f64, (bh, bw), int(filter_size), mesh, work, bkg, rms,
                      {} if nsigma is None else {float(nsigma): thr})


def estimate_background(frame, box=(64, 64), filter_size=3, mask=None, exclude=None, sigma=3.0, max_iters=10,
                        min_good_fraction=0.5):
    """Sky background and noise maps of ``frame``, on the device (``spx_background_mesh_*`` +
    ``spx_background_maps_*``; the definitions are in ``include/subpixal_hip.h``).

    frame : 2-D numpy array or CUDA tensor; float64 frames are processed in float64, everything else in float32.
    box : (height, width) of a mesh cell, 8..128 a side, at most 16384 pixels (float64 frames: 8192).
    filter_size : side of the median filter over the mesh, 1, 3, 5 or 7.
    mask : booleans ``[ny, nx]``, True = bad, or None.
    exclude : int32 label image (a ``Sources.segmentation``): pixels with a label are left out.
    sigma, max_iters : the clipping ``med +- sigma * std`` of each cell's values and its most rounds (0: none).
    min_good_fraction : a cell with fewer usable pixels than this share of its pixels (or fewer than 2) is bad
        and filled from its neighbours.

    Returns a :class:`Background`; raises ``SubpixalHipError`` when no cell of the mesh is good.  All results are
    bit-identical from run to run."""
    return _estimate_background(frame, box, filter_size, mask, exclude, sigma, max_iters, min_good_fraction)


def detect_sources(frame, nsigma=1.5, box=(64, 64), filter_size=3, mask=None, sigma=3.0, max_iters=10,
                   min_good_fraction=0.5, passes=1, errors=False, gain=None, **find_sources_kwargs):
    """:func:`estimate_background`, then :func:`find_sources` with ``threshold = background + nsigma * rms`` and
    that background, without the frame leaving the device.  ``passes=2`` estimates the background again with the
    sources of the first pass excluded and detects again.  ``find_sources_kwargs``: ``filter_kernel``,
    ``min_area``, ``connectivity``, ``deblend``, ``deblend_levels``, ``deblend_contrast``, ``deblend_mode``.
    ``errors=True`` also measures the errors of the final pass's sources with its ``Background.rms`` and ``gain``
    (``find_sources(..., rms=bg.rms, gain=gain)``); off by default, nothing changes then.
    Returns the :class:`Sources` with ``background_model`` attached."""
    if passes not in (1, 2):
        raise ValueError("passes must be 1 or 2.")
    if errors:
        _check_error_arguments(0.0, gain, ())
    elif gain is not None:
        raise ValueError("gain needs errors=True.")
    for k in find_sources_kwargs:
        if k not in ('filter_kernel', 'min_area', 'connectivity', 'deblend', 'deblend_levels', 'deblend_contrast',
                     'deblend_mode'):
            raise TypeError("detect_sources() got an unexpected keyword argument %r" % k)
    fshape = frame if isinstance(frame, torch.Tensor) else np.asarray(frame)
    _check_background_arguments(fshape, box, filter_size, mask, None, sigma, max_iters, min_good_fraction,
                                _is_f64(frame))
    _check_arguments(fshape, mask, None if find_sources_kwargs.get('filter_kernel') is None
                     else np.asarray(find_sources_kwargs['filter_kernel']), find_sources_kwargs.get('min_area', 5),
                     find_sources_kwargs.get('connectivity', 8))
    if find_sources_kwargs.get('deblend', False):
        _check_deblend_arguments(find_sources_kwargs.get('deblend_levels', 31),
                                 find_sources_kwargs.get('deblend_contrast', 0.005),
                                 find_sources_kwargs.get('deblend_mode', 'exponential'))
    frame = device.to_device(frame, torch.float64 if _is_f64(frame) else torch.float32)       # the one upload
    mask = None if mask is None else device.to_device(mask, torch.uint8)
    exclude, src = None, None
    for i in range(passes):
        bg = _estimate_background(frame, box, filter_size, mask, exclude, sigma, max_iters, min_good_fraction,
                                  nsigma=float(nsigma))
        last = errors and i == passes - 1
        src = find_sources(frame, bg.threshold(nsigma), background=bg.background, mask=mask,
                           rms=bg.rms if last else None, gain=gain if last else None, **find_sources_kwargs)
        exclude = src.segmentation
    src.background_model = bg
    return src
