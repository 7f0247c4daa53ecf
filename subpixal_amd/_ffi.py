"""ctypes binding of libsubpixal_hip.so (include/subpixal_hip.h).

There is no CPU fallback: importing this module without the built library, or
calling into it without an MI355X visible, raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SPX_HIP_LIB: another build of the same library (A/B measurements only: tools/gpu_r3_variants.sh)
LIB_PATH = os.environ.get('SPX_HIP_LIB') or os.path.join(_HERE, 'csrc', 'libsubpixal_hip.so')

ABI_VERSION = 4
MEASURE_COLUMNS = 13                                     # SPX_MEASURE_COLUMNS
ERROR_COLUMNS = 6                                        # SPX_ERROR_COLUMNS
DRIZZLE_ROW_BYTES = 224                                  # SPX_DRIZZLE_ROW_BYTES
DRIZZLE_POLY_ROW_BYTES = 488                             # SPX_DRIZZLE_POLY_ROW_BYTES
# byte offsets of a packed polynomial row's fields (csrc/spx_drizzle_poly_kernels.h: DrizzlePolyRow): coef [2][21],
# the frame's centre, A^-1, the window (rx, ry), the drop bounds (bx, by), degree and steps (two int32)
DRIZZLE_POLY_ROW_COEF, DRIZZLE_POLY_ROW_CENTER, DRIZZLE_POLY_ROW_INV = 40, 376, 392
DRIZZLE_POLY_ROW_WINDOW, DRIZZLE_POLY_ROW_DROP, DRIZZLE_POLY_ROW_DEGREE = 424, 456, 480
E_ARG, E_SHAPE = -1, -2                                  # SPX_E_ARG, SPX_E_SHAPE
E_WORKSPACE = -4                                         # SPX_E_WORKSPACE
SKY_STATS = {'median': 0, 'mean': 1, 'mode': 2}          # SPX_SKY_MEDIAN / _MEAN / _MODE
SKY_EMPTY, SKY_BAD_FRAME = 1, 2                          # SPX_SKY_EMPTY, SPX_SKY_BAD_FRAME
REFINE_DEFAULT, REFINE_F64, REFINE_F32 = 0, 1, 2         # SPX_REFINE_* (include/subpixal_hip.h)
MAX_SIDE = 682
MAX_UPSAMPLE = 59
MAX_UPSAMPLE_GENERAL = 39      # cutouts above 128 px

CC_CODES = {'CC': 0, 'NCC': 1, 'ZNCC': 2}

ST_OK, ST_EDGE, ST_NOMAX, ST_OUTSIDE, ST_WINDOW, ST_FEWPTS, ST_NONFINITE, ST_SHAPE = range(8)

_c = ctypes
_vp = _c.c_void_p
_SIGNATURES = {
    'spx_abi_version': (_c.c_int, []),
    'spx_device_count': (_c.c_int, []),
    'spx_init': (_c.c_int, [_c.c_int]),
    'spx_prepare': (_c.c_int, [_c.c_int]),
    'spx_prepare_shape': (_c.c_int, [_c.c_int, _c.c_int, _c.c_int]),
    'spx_shutdown': (_c.c_int, []),
    'spx_last_error': (_c.c_char_p, []),
    'spx_workspace_bytes_xcorr': (_c.c_size_t, [_c.c_int64, _c.c_int, _c.c_int]),
    'spx_workspace_bytes_displacement5': (_c.c_size_t, [_c.c_int64, _c.c_int, _c.c_int, _c.c_int]),
    'spx_xcorr_refine_f32': (_c.c_int, [_vp, _vp, _c.c_int64, _c.c_int, _c.c_int, _c.c_int,
                                        _c.c_int, _vp, _vp, _vp, _c.c_size_t, _vp]),
    'spx_xcorr_refine_f64': (_c.c_int, [_vp, _vp, _c.c_int64, _c.c_int, _c.c_int, _c.c_int,
                                        _c.c_int, _vp, _vp, _vp, _c.c_size_t, _vp]),
    # ... with the refine stage's arithmetic chosen per call (REFINE_DEFAULT / REFINE_F64)
    'spx_xcorr_refine_ex_f32': (_c.c_int, [_vp, _vp, _c.c_int64, _c.c_int, _c.c_int, _c.c_int,
                                           _c.c_int, _c.c_int, _vp, _vp, _vp, _c.c_size_t, _vp]),
    'spx_xcorr_refine_ex_f64': (_c.c_int, [_vp, _vp, _c.c_int64, _c.c_int, _c.c_int, _c.c_int,
                                           _c.c_int, _c.c_int, _vp, _vp, _vp, _c.c_size_t, _vp]),
    'spx_find_displacement5_f32': (_c.c_int, [_vp, _vp, _c.c_int64, _c.c_int, _c.c_int,
                                              _c.c_int, _vp, _vp, _vp, _vp, _c.c_size_t, _vp]),
    'spx_find_displacement5_f64': (_c.c_int, [_vp, _vp, _c.c_int64, _c.c_int, _c.c_int,
                                              _c.c_int, _vp, _vp, _vp, _vp, _c.c_size_t, _vp]),
    'spx_find_displacement5_var_f32': (_c.c_int, [_vp, _vp, _vp, _vp, _c.c_int64, _c.c_int, _c.c_int, _vp, _vp,
                                                  _vp, _vp, _c.c_size_t, _vp]),
    'spx_find_displacement5_var_f64': (_c.c_int, [_vp, _vp, _vp, _vp, _c.c_int64, _c.c_int, _c.c_int, _vp, _vp,
                                                  _vp, _vp, _c.c_size_t, _vp]),
    'spx_find_displacement5_catalog_f32': (_c.c_int, [_vp, _vp, _vp, _vp, _c.c_int64, _c.c_int, _c.c_int, _vp, _vp,
                                                      _vp, _vp, _c.c_size_t, _vp]),
    # ... for float64 cutouts and blots (out_icc stays float32)
    'spx_find_displacement5_catalog_f64': (_c.c_int, [_vp, _vp, _vp, _vp, _c.c_int64, _c.c_int, _c.c_int, _vp, _vp,
                                                      _vp, _vp, _c.c_size_t, _vp]),
    'spx_gather_cutouts_var_f32': (_c.c_int, [_vp, _vp, _c.c_int, _c.c_int, _vp, _c.c_int64, _vp, _c.c_float,
                                              _vp, _vp, _vp, _vp]),
    'spx_gather_cutouts_var_f64': (_c.c_int, [_vp, _vp, _c.c_int, _c.c_int, _vp, _c.c_int64, _vp, _c.c_double,
                                              _vp, _vp, _vp, _vp]),
    'spx_blot4_var_f32': (_c.c_int, [_vp, _vp, _vp, _c.c_int64, _vp, _c.c_int, _vp, _vp, _vp, _vp, _vp]),
    # ... the same float32 blots stored as float64 (for float64 image cutouts)
    'spx_blot4_var_to_f64': (_c.c_int, [_vp, _vp, _vp, _c.c_int64, _vp, _c.c_int, _vp, _vp, _vp, _vp, _vp]),
    'spx_find_peak_f64': (_c.c_int, [_vp, _vp, _vp, _c.c_int64, _c.c_int, _c.c_int, _c.c_int,
                                     _c.c_int, _c.c_int, _c.c_int, _vp, _vp, _vp]),
    'spx_gather_cutouts_f32': (_c.c_int, [_vp, _vp, _c.c_int, _c.c_int, _vp, _c.c_int64,
                                          _c.c_int, _c.c_int, _c.c_float, _vp, _vp, _vp, _vp]),
    'spx_gather_cutouts_f64': (_c.c_int, [_vp, _vp, _c.c_int, _c.c_int, _vp, _c.c_int64,
                                          _c.c_int, _c.c_int, _c.c_double, _vp, _vp, _vp, _vp]),
    'spx_label_bboxes_i32': (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int32, _vp, _vp, _vp]),
    # source finding: segmentation image (spx_detect_label_*) and isophotal measurements (spx_measure_labels_*)
    'spx_detect_workspace_bytes': (_c.c_size_t, [_c.c_int, _c.c_int]),
    'spx_detect_label_f32': (_c.c_int, [_vp, _vp, _c.c_float, _vp, _vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                        _c.c_int, _c.c_int, _vp, _c.c_size_t, _vp, _vp, _vp]),
    'spx_detect_label_f64': (_c.c_int, [_vp, _vp, _c.c_double, _vp, _vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                        _c.c_int, _c.c_int, _vp, _c.c_size_t, _vp, _vp, _vp]),
    'spx_measure_labels_f32': (_c.c_int, [_vp, _vp, _c.c_double, _vp, _vp, _c.c_int, _c.c_int, _c.c_int, _vp, _vp,
                                          _vp, _vp]),
    'spx_measure_labels_f64': (_c.c_int, [_vp, _vp, _c.c_double, _vp, _vp, _c.c_int, _c.c_int, _c.c_int, _vp, _vp,
                                          _vp, _vp]),
    # per-source errors (spx_measure_errors_*): frame, mask, bkg, bkg_map, rms, rms_map, gain, labels, fny, fnx,
    # nlabels, boxes, the measure table, out_errors, out_eflags, stream
    'spx_measure_errors_f32': (_c.c_int, [_vp, _vp, _c.c_double, _vp, _c.c_double, _vp, _c.c_double, _vp, _c.c_int,
                                          _c.c_int, _c.c_int, _vp, _vp, _vp, _vp, _vp]),
    'spx_measure_errors_f64': (_c.c_int, [_vp, _vp, _c.c_double, _vp, _c.c_double, _vp, _c.c_double, _vp, _c.c_int,
                                          _c.c_int, _c.c_int, _vp, _vp, _vp, _vp, _vp]),
    # drizzle: spx_drizzle_rows packs HOST tables (frames, weights, masks, shapes, maps, active, nframes, pixfrac,
    # kernel, out_ny, out_nx, out_rows); spx_drizzle_*: device rows, nframes, kernel, fill, out_ny, out_nx, sci, wht,
    # ctx, stream
    'spx_drizzle_rows': (_c.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _c.c_int, _c.c_double, _c.c_int, _c.c_int, _c.c_int,
                                    _vp]),
    'spx_drizzle_f32': (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_double, _c.c_int, _c.c_int, _vp, _vp, _vp, _vp]),
    'spx_drizzle_f64': (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_double, _c.c_int, _c.c_int, _vp, _vp, _vp, _vp]),
    # drizzle through polynomial maps: spx_drizzle_poly_rows packs HOST tables (frames, weights, masks, shapes, coef
    # [K][2][21], degree [K], center [K][2], active, nframes, pixfrac, kernel, out_ny, out_nx, out_rows);
    # spx_drizzle_poly_*: as spx_drizzle_*
    'spx_drizzle_poly_rows': (_c.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c.c_int, _c.c_double, _c.c_int,
                                         _c.c_int, _c.c_int, _vp]),
    'spx_drizzle_poly_f32': (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_double, _c.c_int, _c.c_int, _vp, _vp, _vp, _vp]),
    'spx_drizzle_poly_f64': (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_double, _c.c_int, _c.c_int, _vp, _vp, _vp, _vp]),
    # cosmic-ray rejection.  spx_drizzle_median_*: device rows, nframes, nactive, kernel, nlow, nhigh, out_ny, out_nx,
    # med, nmed, stream; spx_drizzle_cr_*: device rows, nframes, frame, fny, fnx, med, nmed, out_ny, out_nx, rms,
    # rms_map, sky, gain, snr1, snr2, scale1, scale2, crmask, clean, stream
    'spx_drizzle_median_f32': (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                          _vp, _vp, _vp]),
    'spx_drizzle_median_f64': (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                          _vp, _vp, _vp]),
    'spx_drizzle_cr_f32': (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _vp, _vp, _c.c_int, _c.c_int,
                                      _c.c_double, _vp, _c.c_double, _c.c_double, _c.c_double, _c.c_double,
                                      _c.c_double, _c.c_double, _vp, _vp, _vp]),
    'spx_drizzle_cr_f64': (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _vp, _vp, _c.c_int, _c.c_int,
                                      _c.c_double, _vp, _c.c_double, _c.c_double, _c.c_double, _c.c_double,
                                      _c.c_double, _c.c_double, _vp, _vp, _vp]),
    # minmed and the mask growth.  spx_drizzle_minmed_*: device rows, nframes, nactive, kernel, nlow, nhigh, device
    # table [K][3], nsigma1, nsigma2, grow, out_ny, out_nx, md, lo, bits, med, nmed, minmed, stream;
    # spx_drizzle_cr_grow_*: device rows, nframes, frame, fny, fnx, med, nmed, out_ny, out_nx, rms, rms_map, seed,
    # grow, ctegrow, ctedir, crmask, clean, stream
    'spx_drizzle_minmed_f32': (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _vp, _c.c_double,
                                          _c.c_double, _c.c_int, _c.c_int, _c.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                          _vp]),
    'spx_drizzle_minmed_f64': (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _vp, _c.c_double,
                                          _c.c_double, _c.c_int, _c.c_int, _c.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                          _vp]),
    'spx_drizzle_cr_grow_f32': (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _vp, _vp, _c.c_int, _c.c_int,
                                           _c.c_double, _vp, _vp, _c.c_int, _c.c_int, _c.c_int, _vp, _vp, _vp]),
    'spx_drizzle_cr_grow_f64': (_c.c_int, [_vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _vp, _vp, _c.c_int, _c.c_int,
                                           _c.c_double, _vp, _vp, _c.c_int, _c.c_int, _c.c_int, _vp, _vp, _vp]),
    # deblending of merged sources (spx_deblend_labels_*): frame, mask, filter, fky, fkx, fny, fnx, labels,
    # nlabels, boxes, connectivity, min_area, nlevels, contrast, mode, work, work_bytes, out_labels, out_parent,
    # out_dflags, max_out, out_nlabels, stream
    'spx_deblend_workspace_bytes': (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int]),
    'spx_deblend_labels_f32': (_c.c_int, [_vp, _vp, _vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _vp, _c.c_int, _vp,
                                          _c.c_int, _c.c_int, _c.c_int, _c.c_double, _c.c_int, _vp, _c.c_size_t,
                                          _vp, _vp, _vp, _c.c_int, _vp, _vp]),
    'spx_deblend_labels_f64': (_c.c_int, [_vp, _vp, _vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _vp, _c.c_int, _vp,
                                          _c.c_int, _c.c_int, _c.c_int, _c.c_double, _c.c_int, _vp, _c.c_size_t,
                                          _vp, _vp, _vp, _c.c_int, _vp, _vp]),
    # sky background: per-cell statistics (spx_background_mesh_*), filtered mesh -> maps (spx_background_maps_*)
    'spx_background_workspace_bytes': (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    'spx_background_mesh_f32': (_c.c_int, [_vp, _vp, _vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_double,
                                           _c.c_int, _c.c_double, _vp, _vp, _vp, _vp]),
    'spx_background_mesh_f64': (_c.c_int, [_vp, _vp, _vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_double,
                                           _c.c_int, _c.c_double, _vp, _vp, _vp, _vp]),
    'spx_background_maps_f32': (_c.c_int, [_vp, _vp, _vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                           _c.c_int, _c.c_double, _vp, _c.c_size_t, _vp, _vp, _vp, _vp, _vp]),
    'spx_background_maps_f64': (_c.c_int, [_vp, _vp, _vp, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                           _c.c_int, _c.c_double, _vp, _c.c_size_t, _vp, _vp, _vp, _vp, _vp]),
    # whole-frame sigma-clipped statistics (spx_sky_stats_*): DEVICE tables frames, weights, masks, shapes; nframes,
    # lower, upper, lsigma, usigma, max_iters, stat, work, work_bytes, out, out_counts, out_status, stream
    'spx_sky_workspace_bytes': (_c.c_size_t, [_c.c_int]),
    'spx_sky_stats_f32': (_c.c_int, [_vp, _vp, _vp, _vp, _c.c_int, _c.c_double, _c.c_double, _c.c_double, _c.c_double,
                                     _c.c_int, _c.c_int, _vp, _c.c_size_t, _vp, _vp, _vp, _vp]),
    'spx_sky_stats_f64': (_c.c_int, [_vp, _vp, _vp, _vp, _c.c_int, _c.c_double, _c.c_double, _c.c_double, _c.c_double,
                                     _c.c_int, _c.c_int, _vp, _c.c_size_t, _vp, _vp, _vp, _vp]),
    'spx_blot_affine4_f32': (_c.c_int, [_vp, _c.c_int64, _c.c_int, _c.c_int, _vp, _vp, _c.c_int,
                                        _c.c_int, _vp, _vp]),
    'spx_blot_poly4_f32': (_c.c_int, [_vp, _c.c_int64, _c.c_int, _c.c_int, _vp, _c.c_int, _vp, _c.c_int,
                                      _c.c_int, _vp, _vp]),
    'spx_gen_gaussian_pairs_f32': (_c.c_int, [_c.c_uint64, _c.c_int64, _c.c_int64, _c.c_int,
                                              _c.c_float, _c.c_float, _c.c_float, _vp, _vp,
                                              _vp, _vp]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


class SubpixalHipError(RuntimeError):
    """A call into libsubpixal_hip.so returned an error code."""


def load():
    """Load (once) and return the ctypes library; raises if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libsubpixal_hip.so is not built (%s); run `python -c 'import "
                "__graft_entry__ as g; g.build()'` or `make -C subpixal_amd/csrc`. "
                "subpixal_amd has no CPU fallback." % LIB_PATH)
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)       # AttributeError if a symbol is missing
            fn.restype = res
            fn.argtypes = args
        if lib.spx_abi_version() != ABI_VERSION:
            raise ImportError("libsubpixal_hip.so ABI version mismatch")
        _lib = lib
    return _lib


def check(rc):
    if rc != 0:
        msg = load().spx_last_error()
        raise SubpixalHipError("libsubpixal_hip error %d: %s"
                               % (rc, msg.decode() if msg else ''))
