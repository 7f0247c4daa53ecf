"""Catalogues of sources found on the device, with the reference's selection language.

:class:`DeviceImageCatalog` carries the interface of the reference's ``ImageCatalog`` / ``SExImageCatalog``
(``catalogs.py``) wherever it has a meaning without FITS files and SExtractor: the image is a frame (numpy array
or CUDA tensor), the source finder is :func:`subpixal_amd.detect.detect_sources` with ``errors=True``, and the
catalogue is a dict of equal-length numpy columns under the reference's column names (``id, x, y, flux, fluxerr,
semi-major-a, semi-major-b, fwhm`` plus the derived ``pos_std, weight``; there is no stellarity column).  The
selection itself -- source mask, ``(column, op, value)`` filters, top/bottom-N -- is :func:`select`, a restatement
of ``SExImageCatalog.execute`` (catalogs.py:814-899) on the host: the columns are small.

    cat = catalogs.DeviceImageCatalog(frame, nsigma=5.0, min_area=5)
    cat.append_filters([('flux', 'h', 2000), ('pos_std', '<', 0.05)])
    cat.execute()
    drz_cat = cat.cutout_catalog(frame, pad=9)             # src_weight = 1 / pos_std**2
"""
import numpy as np

from . import detect
from .utils import py2round

__all__ = ['DeviceImageCatalog', 'select', 'REQUIRED_COLNAMES', 'DERIVED_COLNAMES']

REQUIRED_COLNAMES = ('id', 'x', 'y', 'flux', 'fluxerr', 'semi-major-a', 'semi-major-b', 'fwhm')
DERIVED_COLNAMES = ('pos_std', 'weight')
DEFAULT_FILTERS = (('flux', '>', 0), ('fwhm', '>', 0), ('semi-major-a', '>', 0), ('semi-major-b', '>', 0))


def _select_high(values, nrows):
    """The reference's ``'h'`` (catalogs.py:40-45): rows sorted by value, ascending and stable (ties keep catalogue
    order); ``nrows >= 0`` keeps the last ``nrows`` of that order -- and ``nrows == 0`` all of them, since the
    reference slices ``[-nrows:]`` --, a negative ``nrows`` keeps the FIRST ``-nrows`` of it, i.e. shuts out the
    highest ``len - |nrows|`` rows."""
    idx = np.argsort(np.asarray(values), kind='stable')
    idx = idx[-nrows:] if nrows >= 0 else idx[:-nrows]
    mask = np.zeros(len(values), bool)
    mask[idx] = True
    return mask


def _select_lower(values, nrows):
    """The reference's ``'l'`` (catalogs.py:48-53): the first ``nrows`` of the same order; a negative ``nrows`` keeps
    the LAST ``-nrows`` of it."""
    idx = np.argsort(np.asarray(values), kind='stable')
    idx = idx[:nrows] if nrows >= 0 else idx[nrows:]
    mask = np.zeros(len(values), bool)
    mask[idx] = True
    return mask


CMP_MAP = {'>': np.greater, '>=': np.greater_equal, '==': np.equal, '!=': np.not_equal, '<': np.less,
           '<=': np.less_equal, 'h': _select_high, 'l': _select_lower}


def _norm_op(op):
    op = ''.join(str(op).split())
    if op not in CMP_MAP:
        raise ValueError("unknown comparison %r: use one of %s." % (op, ', '.join(sorted(CMP_MAP))))
    return op


def _take(catalog, rows):
    return {k: v[rows] for k, v in catalog.items()}


def _compare(catalog, filters, keep, ranked):
    for key, op, val in filters:
        if (op in ('h', 'l')) == ranked and key in catalog:
            keep = keep & CMP_MAP[op](catalog[key], val)
    return keep


def select(raw, filters, mask=None, mask_type=None, required=REQUIRED_COLNAMES, position_std=None, weights=None):
    """The rows of ``raw`` (dict of equal-length columns) that pass, in the order of catalogs.py:814-899:

    1. rows with a non-finite value in a ``required`` column are dropped (the reference drops masked values);
    2. the source mask, looked up at ``(py2round(x), py2round(y))`` (positions are 0-based here, so nothing is
       subtracted first): ``mask_type='coords'``, an ``[N, 2]`` list of (x, y), drops a source that sits on a
       listed pixel; ``'image'``, booleans ``[ny, nx]``, drops a source on a True pixel AND one whose rounded
       position lies outside the mask image;
    3. the comparison filters;
    4. the derived columns ``pos_std = position_std(catalog)``, ``weight = weights(catalog)`` (skipped when the
       function is None or returns None);
    5. the comparison filters again, now that ``pos_std`` and ``weight`` exist;
    6. the ``'h'`` / ``'l'`` filters, each ranked over the rows that are left and all of them ANDed.
    A filter on a column the catalogue does not have is skipped.  Returns a new dict of columns."""
    raw = {k: np.asarray(v) for k, v in raw.items()}
    n = len(next(iter(raw.values()))) if raw else 0
    filters = [(k, _norm_op(o), v) for k, o, v in (f[:3] for f in filters)]
    keep = np.ones(n, bool)
    for c in required:
        if c in raw and np.issubdtype(raw[c].dtype, np.floating):
            keep &= np.isfinite(raw[c])
    catalog = _take(raw, keep)
    m = int(keep.sum())
    if 'x' in catalog and 'y' in catalog:
        xi = py2round(np.asarray(catalog['x'], np.float64)).astype(np.int64)
        yi = py2round(np.asarray(catalog['y'], np.float64)).astype(np.int64)
    elif mask is not None:
        raise ValueError("a source mask needs the columns 'x' and 'y'.")
    if mask is None:
        keep = np.ones(m, bool)
    elif mask_type == 'coords':
        listed = {(int(a), int(b)) for a, b in np.asarray(mask)}
        keep = np.array([(int(a), int(b)) not in listed for a, b in zip(xi, yi)], bool).reshape(m)
    elif mask_type == 'image':
        ymmax, xmmax = mask.shape
        inside = (xi >= 0) & (xi < xmmax) & (yi >= 0) & (yi < ymmax)
        keep = np.zeros(m, bool)
        keep[inside] = ~np.asarray(mask, bool)[yi[inside], xi[inside]]
    else:
        raise ValueError("mask_type must be 'coords' or 'image' when a mask is given.")
    catalog = _take(catalog, _compare(catalog, filters, keep, ranked=False))
    if position_std is not None:
        pos_std = position_std(catalog)
        if pos_std is not None:
            catalog['pos_std'] = np.asarray(pos_std)
    if weights is not None:
        w = weights(catalog)
        if w is not None:
            catalog['weight'] = np.asarray(w)
    n2 = len(next(iter(catalog.values()))) if catalog else 0
    catalog = _take(catalog, _compare(catalog, filters, np.ones(n2, bool), ranked=False))
    n3 = len(next(iter(catalog.values()))) if catalog else 0
    return _take(catalog, _compare(catalog, filters, np.ones(n3, bool), ranked=True))


class DeviceImageCatalog(object):
    """Find the sources of a frame on the device and select among them as the reference's ``SExImageCatalog`` does.

    image : the frame (2-D numpy array or CUDA tensor), or None: :meth:`set_image` later.
    nsigma, box, filter_size, sigma, max_iters, min_good_fraction, passes, gain, and as keywords filter_kernel,
    min_area, connectivity, deblend, deblend_levels, deblend_contrast, deblend_mode : the detection parameters of
        :func:`detect.detect_sources`, which :meth:`execute` calls with ``errors=True``.
    bad_pixels : the DETECTION mask (booleans ``[ny, nx]``, True = bad pixel), ``detect_sources``'s ``mask``.  Not
        to be confused with :meth:`set_mask`, which masks SOURCES of the catalogue, as in the reference.

    After :meth:`execute`: :attr:`catalog`, :attr:`sources` (the :class:`detect.Sources` of all detections),
    :meth:`get_segmentation_image`, :meth:`cutout_catalog`."""

    def __init__(self, image=None, nsigma=1.5, box=(64, 64), filter_size=3, sigma=3.0, max_iters=10,
                 min_good_fraction=0.5, passes=1, gain=None, bad_pixels=None, **find_sources_kwargs):
        self._detect_kwargs = dict(nsigma=nsigma, box=box, filter_size=filter_size, sigma=sigma, max_iters=max_iters,
                                   min_good_fraction=min_good_fraction, passes=passes, gain=gain, mask=bad_pixels,
                                   **find_sources_kwargs)
        self._filters = []
        self._required_colnames = list(REQUIRED_COLNAMES)
        self._derived_colnames = list(DERIVED_COLNAMES)
        self.set_default_filters()
        self._mask = None
        self._mask_type = None
        self._image = None
        self._dirty_image = False
        self._rawcat = None
        self._sources = None
        self._catalog = self._empty_catalog()
        self.set_image(image)

    def _empty_catalog(self):
        names = self._required_colnames + self._derived_colnames
        return {c: np.zeros(0, np.int64 if c == 'id' else np.float64) for c in names}

    # -- image and raw catalogue ---------------------------------------------------------------------------------
    def set_image(self, image):
        """Set the frame to find sources in; the next :meth:`execute` runs the detection again."""
        self._image = image
        self._dirty_image = image is not None
        self._rawcat, self._sources = None, None
        self._catalog = self._empty_catalog()

    def set_raw_catalog(self, columns, sources=None):
        """Use ``columns`` (dict of equal-length arrays under the reference's column names) as the raw catalogue
        instead of detecting: the counterpart of loading a catalogue file in the reference.  ``sources``: the
        :class:`detect.Sources` they came from, if :meth:`cutout_catalog` is wanted."""
        columns = {k: np.asarray(v) for k, v in columns.items()}
        if len({len(v) for v in columns.values()}) > 1:
            raise ValueError("the columns of a catalogue must have one length.")
        self._rawcat, self._sources = columns, sources
        self._dirty_image = False
        self._catalog = self._empty_catalog()

    @property
    def rawcat(self):
        """The catalogue of all detections, before mask and filters (None before :meth:`execute`)."""
        return self._rawcat

    @property
    def rawcat_colnames(self):
        return None if self._rawcat is None else list(self._rawcat)

    @property
    def sources(self):
        return self._sources

    @property
    def required_colnames(self):
        """The column names a raw catalogue must have."""
        return self._required_colnames[:]

    # -- source mask ---------------------------------------------------------------------------------------------
    @property
    def mask_type(self):
        """'coords', 'image' or None (no mask)."""
        return self._mask_type

    def set_mask(self, mask):
        """Mask of "bad" SOURCES: a boolean image (True = drop the sources whose rounded position falls there), an
        ``[N, 2]`` integer array of (x, y) pixels or a tuple ``(x_list, y_list)`` of them, or None."""
        if mask is None:
            self._mask, self._mask_type = None, None
            return
        if isinstance(mask, tuple):
            if len(mask) != 2:
                raise ValueError("a tuple mask must hold two 1-D lists of integer coordinates.")
            x, y = np.asarray(mask[0]), np.asarray(mask[1])
            if x.ndim != 1 or x.shape != y.shape or not (np.issubdtype(x.dtype, np.integer)
                                                         and np.issubdtype(y.dtype, np.integer)):
                raise ValueError("a tuple mask must hold two 1-D lists of integer coordinates of one length.")
            self._mask, self._mask_type = np.stack([x, y], axis=1), 'coords'
            return
        mask = np.asarray(mask.cpu()) if hasattr(mask, 'cpu') else np.array(mask)
        if mask.ndim == 2 and mask.dtype == np.bool_:
            self._mask, self._mask_type = mask, 'image'
        elif mask.ndim == 2 and mask.shape[1] == 2 and np.issubdtype(mask.dtype, np.integer):
            self._mask, self._mask_type = mask, 'coords'
        else:
            raise ValueError("Unsupported mask type or format.")

    # -- filters -------------------------------------------------------------------------------------------------
    def set_default_filters(self):
        """``flux > 0`` AND ``fwhm > 0`` AND ``semi-major-a > 0`` AND ``semi-major-b > 0``."""
        self._filters = list(DEFAULT_FILTERS)

    @staticmethod
    def _find_filters(filters, key, op=None):
        idxs = [i for i, (k, o, _) in enumerate(filters) if k == key and (op is None or o == op)]
        return idxs or None

    @staticmethod
    def _as_filter(f):
        if not isinstance(f, tuple) or len(f) < 3:
            raise TypeError("a filter is a tuple (colname, op, value).")
        return (f[0], _norm_op(f[1]), f[2])

    def set_filters(self, fcond):
        """Replace the filters by ``fcond``: a tuple ``(colname, op, value)`` or a list of them, ``op`` one of
        ``> >= == != < <= h l``.  ``'h'`` / ``'l'`` keep the ``value`` rows with the highest / lowest ``colname``
        and act last.  Of several filters on one column with one operator, the last one given counts."""
        if isinstance(fcond, list):
            filters = []
            for f in fcond[::-1]:
                key, op, val = self._as_filter(f)
                if self._find_filters(filters, key, op) is None:
                    filters.insert(0, (key, op, val))
        elif isinstance(fcond, tuple):
            filters = [self._as_filter(fcond)]
        else:
            raise TypeError("'fcond' must be a tuple or a list of tuples.")
        self._filters = filters

    def append_filters(self, fcond):
        """Add filters to those set; one on the same column with the same operator replaces the earlier one."""
        if isinstance(fcond, tuple):
            fcond = [fcond]
        elif not isinstance(fcond, list):
            raise TypeError("'fcond' must be a tuple or a list of tuples.")
        for f in fcond:
            key, op, val = self._as_filter(f)
            for i in (self._find_filters(self._filters, key, op) or [])[::-1]:
                del self._filters[i]
            self._filters.append((key, op, val))

    def remove_filter(self, key, op=None):
        """Remove the filters on column ``key`` (with operator ``op`` only, when given)."""
        if op is not None:
            op = _norm_op(op)
        for i in (self._find_filters(self._filters, key, op) or [])[::-1]:
            del self._filters[i]

    def remove_all_filters(self):
        self._filters = []

    @property
    def filters(self):
        """A list of the active filters."""
        return self._filters[:]

    # -- the catalogue -------------------------------------------------------------------------------------------
    def compute_position_std(self, catalog):
        """``fwhm / (2 sqrt(2 ln 2) * flux / fluxerr)`` (catalogs.py:405-428), or None without those columns."""
        if not all(c in catalog for c in ('fwhm', 'flux', 'fluxerr')):
            return None
        return detect.position_std(np.asarray(catalog['fwhm'], np.float64), np.asarray(catalog['flux'], np.float64),
                                   np.asarray(catalog['fluxerr'], np.float64))

    def compute_weights(self, catalog):
        """``1 / pos_std**2`` (catalogs.py:968-987)."""
        pos_std = self.compute_position_std(catalog)
        if pos_std is None:
            return None
        with np.errstate(all='ignore'):
            return 1.0 / pos_std ** 2

    def execute(self):
        """Find the sources (when the image changed), then apply mask and filters: see :func:`select`."""
        if self._dirty_image:
            src = detect.detect_sources(self._image, errors=True, **self._detect_kwargs)
            t = src.table()
            raw = {c: t[c] for c in self._required_colnames}
            raw['id'] = raw['id'].astype(np.int64)
            for c in ('npix', 'theta', 'peak', 'flags', 'snr', 'errx2', 'erry2', 'errxy', 'nhalf'):
                raw[c] = t[c]
            self._rawcat, self._sources = raw, src
            self._dirty_image = False
        if self._rawcat is None:
            return
        missing = [c for c in self._required_colnames if c not in self._rawcat]
        if missing:
            raise ValueError("the raw catalogue lacks the required columns %s." % ', '.join(missing))
        self._catalog = select(self._rawcat, self._filters, self._mask, self._mask_type,
                               required=self._required_colnames, position_std=self.compute_position_std,
                               weights=self.compute_weights)

    @property
    def catalog(self):
        """The catalogue after mask and filters: a dict of equal-length numpy columns."""
        return self._catalog

    def get_segmentation_image(self):
        """int32 CUDA tensor with the segments of ALL detections (a selected source keeps its id), or None."""
        return None if self._sources is None else self._sources.segmentation

    def cutout_catalog(self, frame, pad=1, dtype=np.float32, weight='pos_std', mask=None):
        """:meth:`detect.Sources.cutout_catalog` for the selected rows only; their ids stay those of the full
        segmentation image."""
        if self._sources is None:
            raise ValueError("no sources: call execute() on an image first.")
        return self._sources._cutout_catalog(frame, pad, dtype, weight, mask, np.asarray(self._catalog['id']))
