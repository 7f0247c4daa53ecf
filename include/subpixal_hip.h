/*
 * subpixal_hip.h -- C ABI of libsubpixal_hip.so: the MI355X (gfx950) replacement
 * for subpixal's per-cutout cross-correlation + sub-pixel peak refinement.
 *
 * The reference (spacetelescope/subpixal) is pure Python and has NO native/FFI
 * boundary; the calls below are what a ctypes binding placed at its hot-path
 * call sites would bind (INTEGRATION.md shows the stub):
 *
 *   spx_find_displacement5_f32  <-  cc.find_displacement(ref, im00, im10, im01,
 *                                   im11, cc_type, full_output)   subpixal/cc.py:21-95,
 *                                   called once per source at subpixal/align.py:682-685;
 *                                   here for a whole batch (the loop align.py:656-699
 *                                   carries no state between sources).  _f64: float64 cutouts.
 *   spx_find_displacement5_var_f32 / _f64
 *                               <-  the same loop over sources whose cutouts differ in shape
 *                                   (bounding box + padding per source, cutout.py:159-175), one
 *                                   launch per kernel family.
 *   spx_xcorr_refine_f32 / _f64 <-  the pair / upsample=U form of the same path that
 *                                   BASELINE.json measures (one fftconvolve, cc.py:114,
 *                                   + find_peak, cc.py:86, on a U-times finer grid).
 *   spx_find_peak_f64           <-  centroid.find_peak(image, xmax, ymax, peak_fit_box,
 *                                   peak_search_box, mask)        subpixal/centroid.py:18-236.
 *   spx_gather_cutouts_f32/_f64 <-  Cutout.__init__ slicing/fill  subpixal/cutout.py:737-755
 *                                   + masked-pixel zeroing        subpixal/align.py:661.
 *   spx_label_bboxes_i32        <-  per-source bounding boxes from the segmentation image
 *                                   subpixal/cutout.py:151-160 (one pass for all sources).
 *   spx_detect_label_f32 / _f64, spx_measure_labels_f32 / _f64
 *                               <-  the source finder the reference shells out to (catalogs.py:
 *                                   SExImageCatalog): segmentation image and isophotal measurements.
 *   spx_measure_errors_f32 / _f64
 *                               <-  the same catalogue's FLUXERR_ISO and FWHM_IMAGE columns (catalogs.py:75-93),
 *                                   from which pos_std and the fit weights derive (catalogs.py:405-428, 968-987).
 *   spx_background_mesh_f32 / _f64, spx_background_maps_f32 / _f64
 *                               <-  the same program's background mesh: sky and noise maps, detection threshold.
 *   spx_drizzle_rows, spx_drizzle_f32 / _f64
 *                               <-  Resample.execute / fast_replace_image (resample.py:535-625): the drizzle of
 *                                   the dithered frames, for affine maps; parity with drizzlepac UNPINNED.
 *   spx_drizzle_poly_rows, spx_drizzle_poly_f32 / _f64
 *                               <-  the same drizzle for frames with polynomial distortion maps (degree 1 .. 5).
 *   spx_drizzle_median_f32 / _f64, spx_drizzle_cr_f32 / _f64
 *                               <-  the cosmic-ray rejection of the same execute() (resample.py:366-390): median,
 *                                   blot back, derivative, drizCR; parity with drizzlepac UNPINNED.
 *   spx_sky_stats_f32 / _f64    <-  sky.subtractSky in front of the same execute() (resample.py:359-364): the
 *                                   sigma-clipped level of every whole frame; parity with drizzlepac UNPINNED.
 *   spx_blot_affine4_f32        <-  the four blot_cutout(dzct, imct) calls per source of
 *                                   subpixal/align.py:664-676 (blot.py:79-155, drizzlepac
 *                                   tblot, interp='poly5') for coordinate maps that are
 *                                   affine over a cutout; drizzlepac is not in the reference
 *                                   tree, the quintic is restated from the published (IRAF
 *                                   bipoly5 / Everett) formula: parity UNPINNED.
 *   spx_blot_poly4_f32          <-  the same four blots through a distorted (polynomial, degree
 *                                   <= 5) coordinate map: BlotWCSMap, blot.py:21-76.
 *   spx_gen_gaussian_pairs_f32  --  synthetic workload generator (bench / tests only).
 *
 * Conventions
 *   - All array pointers are DEVICE pointers owned by the caller (e.g. torch
 *     tensors' data_ptr()), contiguous, row-major; nothing returned is owned by
 *     the library.  `stream` is a hipStream_t (NULL = default stream).  Calls
 *     enqueue work and return without synchronising.
 *   - Return value 0 = OK, negative = SPX_E_* ; spx_last_error() gives the text
 *     (thread-local).  Per-item degenerate cases (edge peak, no maximum ...) are
 *     NOT call failures: they are reported in `out_status` (SPX_ST_*), exactly
 *     the early returns of centroid.py:171-172, 218-225, 230-236.
 *   - Constant tables (twiddles, interpolation kernels) are built on first use
 *     per device and upsampling factor; call spx_prepare() up front if the launch
 *     must not allocate (stream capture).  spx_shutdown() frees them.
 *   - Host threads may share a device: enqueues on one device are serialised by the library
 *     (a per-device mutex held only while a launch is issued).
 *   - Dynamic range: the transforms are float32.  The two cutouts of a pair may differ in amplitude
 *     by any factor up to 2^+-100 (they are balanced by an exact power of two before the product), but
 *     in plain CC mode each must keep sum(|pixel|) below ~6e18 (the zero-frequency term of the packed
 *     spectrum, sum(ref) + i sum(img), is squared in float32; NCC/ZNCC normalise first); beyond that
 *     the correlation overflows and the item comes back as SPX_ST_NONFINITE rather than as a wrong
 *     shift.
 *   - Input element types: the _f32 entries take float32 pixels (the type BASELINE.json
 *     measures); the _f64 entries take float64 pixels and form the `!= 0` masks, the pooled
 *     statistics and the normalised pixels of cc.py:131-156 in float64 -- the dtype the
 *     reference computes in for float64 cutouts -- before rounding to float32 for the
 *     transforms.  All arithmetic after staging is float32 (fit: float64) in both.
 */
#ifndef SUBPIXAL_HIP_H
#define SUBPIXAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPX_ABI_VERSION 4

/* cc_type (cc.py:107-111; anything else than NCC/ZNCC means plain CC) */
#define SPX_CC 0
#define SPX_NCC 1
#define SPX_ZNCC 2

/* per-item status */
#define SPX_ST_OK 0        /* quadratic vertex accepted                                  */
#define SPX_ST_EDGE 1      /* arg-max in row/column 0 -> integer peak (centroid.py:171)  */
#define SPX_ST_NOMAX 2     /* no maximum -> centre of the fit box   (centroid.py:218)    */
#define SPX_ST_OUTSIDE 3   /* vertex outside image -> integer peak  (centroid.py:230)    */
#define SPX_ST_WINDOW 4    /* fine peak not bracketed by the refinement window           */
#define SPX_ST_FEWPTS 5    /* find_peak: fewer than 6 usable points (centroid.py:160,186,202) */
#define SPX_ST_SHAPE 7     /* variable-shape batch: item outside the launched kernel family's sizes */
#define SPX_ST_NONFINITE 6 /* a NaN/Inf pixel made the correlation non-finite.  Pair mode: every lag is NaN,
                              result = integer position (0, 0), what numpy.argmax + centroid.py:171 give.
                              Reference mode: NaN ranks as the maximum as in numpy.argmax (centroid.py:114),
                              result = integer position of the FIRST NaN/Inf of the interlaced image     */

/* error codes */
#define SPX_E_ARG (-1)        /* bad argument                              */
#define SPX_E_SHAPE (-2)      /* cutout shape / upsample not supported     */
#define SPX_E_HIP (-3)        /* HIP runtime error                         */
#define SPX_E_WORKSPACE (-4)  /* workspace missing or too small            */

/* largest cutout side and upsampling factor the kernels accept */
#define SPX_MAX_SIDE 682
#define SPX_MAX_UPSAMPLE 59
#ifndef SPX_MAX_UPSAMPLE_GENERAL      /* (overridable only to MEASURE beyond it: tools/general_precision.py) */
#define SPX_MAX_UPSAMPLE_GENERAL 39 /* pair mode on cutouts above 128 px (float32 transforms: see spx_xcorr_refine_f32) */
#endif

int spx_abi_version(void);
int spx_device_count(void);
/* select `device` for this process/thread and build its constant tables */
int spx_init(int device);
/* Build, for the current device, the interpolation tables of `upsample` for EVERY kernel family
 * (cutouts up to 32 / 85 / 128 px) and raise the dynamic-LDS limit of every kernel instance a
 * later spx_xcorr_refine_* (with this upsample) or spx_find_displacement5_* call can dispatch to,
 * whatever its cutout shape and input type: after it such calls neither allocate nor touch
 * function attributes, so they may be issued inside a stream capture. */
int spx_prepare(int upsample);
/* spx_prepare(upsample) plus the tables of the general path (cutouts above 128 px: FFT period and
 * tables depend on the cutout size) for an (ny, nx) cutout. */
int spx_prepare_shape(int ny, int nx, int upsample);
/* Free the device tables of every device this process initialised (after synchronising them);
 * the next call builds them again.  No call may be in flight on another host thread. */
int spx_shutdown(void);
const char* spx_last_error(void);

/*
 * Bytes of device scratch the batched calls need (0 when none).  Cutouts up to 85 px per side
 * are processed entirely in registers/LDS (FFT period 64 up to 32 px, 128 up to 85 px); larger
 * ones (period 192, up to 128 px) keep per-workgroup class planes and the full convolution in a
 * workspace of 435 KiB per resident workgroup (independent of nbatch beyond the grid); the
 * general path (129..682 px, period 64 C with C = 4..16 classes per axis) needs
 * (4 C^2 64^2 + P (P + 4)) floats per workgroup, two workgroups per CU (one above 341 px).
 * For the reference mode `need_icc` adds room for the interlaced images when the
 * caller does not want them back (out_icc == NULL).
 */
size_t spx_workspace_bytes_xcorr(int64_t nbatch, int ny, int nx);
size_t spx_workspace_bytes_displacement5(int64_t nbatch, int ny, int nx, int need_icc);

/*
 * Pair mode.  ref, img: float32 (or float64) [nbatch][ny][nx].  For every pair: linear
 * cross-correlation on the zero-padded grid (FFT period 64 / 128 / 192 for cutouts up to
 * 32 / 85 / 128 px per side: scipy's next_fast_len(2n-1) for n = 32 and 64, above that the
 * smallest multiple of 64 that leaves the 'same' window free of circular aliasing, i.e. the
 * same numbers at every integer lag), arg-max over the flipped
 * 'same' window, U-times trigonometric upsampling around it, 5x5 quadratic fit
 * (find_peak(., 5, 'all')), shift = peak/U - (n-1)//2.
 *   out_dxdy   : float64 [nbatch][2]  (dx, dy)
 *   out_status : int32   [nbatch]     SPX_ST_* ; may be NULL
 * 5 <= ny, nx <= SPX_MAX_SIDE (cutouts above 128 px take the slow general path: the reference's
 * cutouts, bounding box + padding of a segment, have no upper bound, cutout.py:159-175);
 * 1 <= upsample <= SPX_MAX_UPSAMPLE (cutouts above 128 px: <= SPX_MAX_UPSAMPLE_GENERAL).
 *
 * Accuracy (the transforms are float32): the shift is within 1e-3 px of the float64 evaluation of the same
 * definition (oracle/subpixal_oracle.py xcorr_refine) for sources that FIT their cutout -- Gaussian sigma up to
 * min(15 px, smaller side / 6), i.e. FWHM up to 0.4 of the side and 35 px -- on 24..200 px: every noise-free pair
 * measured, at upsample up to 27 with the default refine, and at upsample 28..59 (up to 39 above 128 px) with
 * SPX_REFINE_F64 on 33..85 px (above 85 px the refine is float64 anyway); there the default (float32) refine
 * covers sigma <= 11 px up to upsample 39 and sigma <= 8 px up to 59 (spx_xcorr_refine_ex_* below).  4.6e-4 px
 * and better for sigma 4..6 px at any upsample in either form, which was also measured with 1 % noise (profiles/r03/width_precision_256.txt,
 * width_precision_other_sizes.txt, width_precision.txt, refine_precision.txt, general_precision.txt).
 * It is NOT a bound for every content: the distance grows with the width of the correlation peak times the
 * upsample factor, and sources that fill their cutout leave 1e-3 px for some pairs -- sigma 8..11 px in 32 px:
 * 1..2 of 128 at upsample >= 39; sigma 11..15 px in 48 px: 1 of 128 at upsample 20 and at 59; sigma 15..25 px in
 * 64..128 px: up to 6 % at upsample 59 (worst measured 4.6e-3 px).  Above 128 px it happens from upsample 40 on
 * for sigma 11..25 px (200 px: 9.7e-4 px at upsample 39, 2.1e-3 at 59): hence SPX_MAX_UPSAMPLE_GENERAL.
 */
int spx_xcorr_refine_f32(const float* ref, const float* img, int64_t nbatch, int ny, int nx,
                         int upsample, int cc_type, double* out_dxdy, int32_t* out_status,
                         void* workspace, size_t workspace_bytes, void* stream);
int spx_xcorr_refine_f64(const double* ref, const double* img, int64_t nbatch, int ny, int nx,
                         int upsample, int cc_type, double* out_dxdy, int32_t* out_status,
                         void* workspace, size_t workspace_bytes, void* stream);

/*
 * The same with the arithmetic of the refine stage (the U-times upsampling around the coarse maximum,
 * upsample > 1) chosen by the caller.  The transforms are float32 either way.
 * Cutouts of 33..85 px per side (the 64 tile and its fold path) have two forms of that stage; up to 32 px it is
 * float32, above 85 px float64, whatever `refine` says.
 *   SPX_REFINE_DEFAULT  what spx_xcorr_refine_f32 / _f64 do: float32 matrix products (= SPX_REFINE_F32).
 *   SPX_REFINE_F64      float64 accumulation: closer to the definition, a wider accuracy domain, slower.
 *   SPX_REFINE_F32      float32, said explicitly.
 * Measured on one MI355X against the float64 definition (profiles/r03/refine_precision.txt, width_precision_256.txt;
 * rates: bench_64_u*_refine_f64.json next to bench.json, bench_64_u20.json; default_rule_cost.txt):
 *   - 4..6-px-sigma spots, 64 px, upsample 10 / 20 / 40: float32 5.5e-5 / 1.3e-4 / 1.3e-4 px, float64 1.2e-5 /
 *     2.3e-5 / 4.5e-5 px; float64 costs 14 % / 21 % of the pairs per second at upsample 10 / 20, 29 % at 28..43
 *     (8.8 instead of 6.2 ms per 1e5 pairs) and 40 % from 44 on (19.7 instead of 11.9 ms at 59): 336 / 512 float64
 *     MFMAs per wave instead of 80, and 2..7 / ~143 spilled registers at three / four window blocks
 *     (f64_live3_ab.txt, f64_live4_ab.txt: the form that spills less was slower);
 *   - the distance grows with the WIDTH of the spot (a flatter correlation peak on the fine grid).  Pairs beyond
 *     1e-3 px, of 256 per (size 64 | 85 px, sigma band, upsample) cell, noise-free:
 *       sigma <= 11 px   float32: 0 up to upsample 39, 0..3 at 59                        float64: 0
 *       sigma 11..15 px  float32: 0 up to upsample 27, 5..6 at 39, 25..30 at 59          float64: 0
 *       sigma 15..20 px  float32: 2..7 up to 27, 22..35 at 39, 47..89 at 59              float64: 0..3
 *       sigma 20..25 px  (85 px) float32: 15..33 up to 27, 60 at 39, 111 at 59           float64: 0..15
 *     So float32 (the default) kept every measured pair within 1e-3 px for sigma <= 11 px up to upsample 39 and
 *     for sigma <= 15 px up to upsample 27; float64 for sigma <= 15 px at every upsample.  A caller who refines
 *     wide sources on very fine grids (sigma 11..15 px at upsample >= 28) asks for SPX_REFINE_F64 and pays the
 *     29..40 %; making that the default for everybody was tried and withdrawn once its cost was measured.
 *     For spots that fill the cutout neither form holds 1e-3 px for every pair (float64: up to 6 % of the pairs
 *     at sigma 20..25 px / upsample 59, worst 4.4e-3 px; see the accuracy note above).
 * Any other value: SPX_E_ARG.
 */
#define SPX_REFINE_DEFAULT 0
#define SPX_REFINE_F64 1
#define SPX_REFINE_F32 2
int spx_xcorr_refine_ex_f32(const float* ref, const float* img, int64_t nbatch, int ny, int nx,
                            int upsample, int cc_type, int refine, double* out_dxdy, int32_t* out_status,
                            void* workspace, size_t workspace_bytes, void* stream);
int spx_xcorr_refine_ex_f64(const double* ref, const double* img, int64_t nbatch, int ny, int nx,
                            int upsample, int cc_type, int refine, double* out_dxdy, int32_t* out_status,
                            void* workspace, size_t workspace_bytes, void* stream);

/*
 * Reference mode (cc.find_displacement).  ref: float32 [nbatch][ny][nx];
 * im4: float32 [nbatch][4][ny][nx] in the order image00, image10, image01,
 * image11.  out_icc: float32 [nbatch][2ny][2nx] interlaced cross-correlation
 * images (full_output=True), or NULL; `workspace` must hold
 * spx_workspace_bytes_displacement5(nbatch, ny, nx, out_icc == NULL) bytes (may be NULL
 * when that is 0).
 * 3 <= ny, nx <= SPX_MAX_SIDE.
 */
int spx_find_displacement5_f32(const float* ref, const float* im4, int64_t nbatch, int ny,
                               int nx, int cc_type, double* out_dxdy, int32_t* out_status,
                               float* out_icc, void* workspace, size_t workspace_bytes,
                               void* stream);
int spx_find_displacement5_f64(const double* ref, const double* im4, int64_t nbatch, int ny,
                               int nx, int cc_type, double* out_dxdy, int32_t* out_status,
                               float* out_icc, void* workspace, size_t workspace_bytes,
                               void* stream);

/*
 * Reference mode over cutouts of DIFFERENT shapes in one launch (the reference's cutouts are
 * bounding boxes + padding, one shape per source: cutout.py:159-175, 1023-1031; the loop at
 * align.py:656-699 handles them one by one).  Items are packed back to back:
 *   item_offset : int64 [nbatch]     element offset of item k's reference cutout in `ref`; its four
 *                                    dithers start at 4*item_offset[k] of `im4` (image00, 10, 01, 11,
 *                                    ny*nx apart), its interlaced image at 4*item_offset[k] of `out_icc`
 *   item_shape  : int32 [nbatch][2]  (ny, nx) of item k
 *   family_side : any side length of the kernel family every item belongs to: items up to 32 px
 *                 with items up to 32 px, up to 64 with up to 64, up to 85 with up to 85, up to 128
 *                 with up to 128 (a family also takes every smaller shape; the Python layer groups
 *                 by the smallest one).  An item outside [3, family maximum] is not computed:
 *                 (NaN, NaN), status SPX_ST_SHAPE.
 *   out_icc     : required (float32, 4 * total pixels); workspace: spx_workspace_bytes_xcorr(nbatch,
 *                 family_side, family_side) bytes.
 * Cutouts above 128 px (general path: tables depend on the size) go through the uniform entry.
 */
int spx_find_displacement5_var_f32(const float* ref, const float* im4, const int64_t* item_offset,
                                   const int32_t* item_shape, int64_t nbatch, int family_side,
                                   int cc_type, double* out_dxdy, int32_t* out_status, float* out_icc,
                                   void* workspace, size_t workspace_bytes, void* stream);
int spx_find_displacement5_var_f64(const double* ref, const double* im4, const int64_t* item_offset,
                                   const int32_t* item_shape, int64_t nbatch, int family_side,
                                   int cc_type, double* out_dxdy, int32_t* out_status, float* out_icc,
                                   void* workspace, size_t workspace_bytes, void* stream);

/*
 * General find_peak (centroid.py:18-236), one image per workgroup.
 *   image : float64 [nbatch][ny][nx]
 *   mask  : uint8   [nbatch][ny][nx] (non-zero = good pixel) or NULL
 *   guess : float64 [nbatch][2] (xmax, ymax) or NULL (search the whole image)
 *   fit box (fit_wx, fit_wy) >= 1; search box (search_wx, search_wy), both 0 =
 *   no brute-force search ('off'/None); ignored when guess is NULL.
 *   out_xy : float64 [nbatch][2]; out_status int32 [nbatch] or NULL.
 */
int spx_find_peak_f64(const double* image, const uint8_t* mask, const double* guess,
                      int64_t nbatch, int ny, int nx, int fit_wx, int fit_wy, int search_wx,
                      int search_wy, double* out_xy, int32_t* out_status, void* stream);

/*
 * Cutout packing: gathers nbatch windows out of a frame into fixed tiles.
 *   frame : float32 [fny][fnx];  fmask: uint8 [fny][fnx] non-zero = bad pixel, or NULL
 *   boxes : int32 [nbatch][4] = (x0, y0, width, height), window may overhang the frame
 *   tiles : float32 [nbatch][tny][tnx]; pixels outside the window/frame, masked
 *           or non-finite are written as `fill` (cutout.py:737,755; align.py:661 uses 0)
 *   seg   : int32 [fny][fnx] segmentation image and ids: int32 [nbatch] the label of each
 *           box's source, or both NULL; with them, pixels of other labels are `fill` as well
 *           (cutout.py:190: mask |= ~(segmentation == sid)).
 */
int spx_gather_cutouts_f32(const float* frame, const uint8_t* fmask, int fny, int fnx,
                           const int32_t* boxes, int64_t nbatch, int tny, int tnx, float fill,
                           float* tiles, const int32_t* seg, const int32_t* ids, void* stream);
/* The same for a float64 frame: frame, fill and tiles are float64 (the reference's Cutout keeps the data's
 * dtype, cutout.py:698-701); everything else as spx_gather_cutouts_f32. */
int spx_gather_cutouts_f64(const double* frame, const uint8_t* fmask, int fny, int fnx,
                           const int32_t* boxes, int64_t nbatch, int tny, int tnx, double fill,
                           double* tiles, const int32_t* seg, const int32_t* ids, void* stream);

/*
 * Bounding boxes of every segment of a label image in one pass (replaces the per-source
 * `segmentation_image == sid` + np.where scans of cutout.py:151-160).
 *   seg    : int32 [fny][fnx], 0 = background, labels 1..max_label (others ignored)
 *   boxes  : int32 [max_label + 1][4] = (xmin, ymin, xmax, ymax), inclusive;
 *            labels without pixels get (INT32_MAX, INT32_MAX, -1, -1)
 *   counts : int32 [max_label + 1] pixels per label
 */
int spx_label_bboxes_i32(const int32_t* seg, int fny, int fnx, int32_t max_label,
                         int32_t* boxes, int32_t* counts, void* stream);

/*
 * Source finding (what the reference leaves to SExtractor, catalogs.py: SExImageCatalog): detection
 * threshold -> connected-component labelling -> minimum area -> labels 1..L in raster order of each
 * component's first pixel, i.e. the numbering of scipy.ndimage.label followed by dropping the small
 * components and closing the gaps.
 *   detected(y,x) = finite(v) && !bad_mask(y,x) && f(y,x) > thr(y,x)          (strict >)
 *   frame      : float32 / float64 [fny][fnx];  bad_mask : uint8 [fny][fnx] (non-zero = bad) or NULL
 *   thr        : thr_map (FLOAT32 [fny][fnx], for both entries) when given, else thr_scalar
 *   filter     : NULL (f = v; fky = fkx = 1), or [fky][fkx] weights in the frame's dtype, odd sides <= 7,
 *                centred: f(y,x) = sum_j sum_i filter[j][i] v'(y + j - fky/2, x + i - fkx/2), where v' = 0
 *                for pixels outside the frame, masked or not finite.  The weights are used as given (the
 *                caller normalises them; nothing is renormalised where pixels drop out); the sum is one
 *                fused multiply-add chain in the frame's dtype, row-major over the filter.
 *   connectivity : 8 or 4;  min_area >= 1: components with fewer pixels are erased (label 0)
 *   work       : spx_detect_workspace_bytes(fny, fnx) bytes of device memory (two int32 frames for the
 *                roots and the per-root counts, the scan's partial sums, a status word); too small or
 *                NULL: SPX_E_WORKSPACE, and nothing is written
 *   out_labels : int32 [fny][fnx] (also holds the parent links while components are merged)
 *   out_nlabels: int32 [1] on the DEVICE: L, or -1 if a merge chain failed its consistency check (no
 *                schedule can produce that from valid inputs; out_labels is undefined then)
 * SPX_E_ARG: null pointer, connectivity not 4 / 8, even filter side or side > 7, min_area < 1;
 * SPX_E_SHAPE: fny or fnx < 1, or fny * fnx >= 2^31 - 1.  Results do not depend on scheduling.
 */
size_t spx_detect_workspace_bytes(int fny, int fnx);
int spx_detect_label_f32(const float* frame, const uint8_t* bad_mask, float thr_scalar, const float* thr_map,
                         const float* filter, int fky, int fkx, int fny, int fnx, int connectivity,
                         int min_area, void* work, size_t work_bytes, int32_t* out_labels,
                         int32_t* out_nlabels, void* stream);
int spx_detect_label_f64(const double* frame, const uint8_t* bad_mask, double thr_scalar, const float* thr_map,
                         const double* filter, int fky, int fkx, int fny, int fnx, int connectivity,
                         int min_area, void* work, size_t work_bytes, int32_t* out_labels,
                         int32_t* out_nlabels, void* stream);

/*
 * Isophotal measurements of labels 1..nlabels of a label image, on the UNFILTERED frame, with
 * w = v - bkg (bkg_map in the frame's dtype when given, else bkg_scalar) over the label's pixels.
 *   boxes         : int32 [nlabels + 1][4], the table spx_label_bboxes_i32 writes (row = label)
 *   out_table_f64 : float64 [nlabels][SPX_MEASURE_COLUMNS], row l - 1 = (npix, flux, x, y, x2, y2, xy, a, b,
 *                   theta, peak, xpeak, ypeak): flux = sum w; x, y = flux-weighted centre (0-based pixel
 *                   centres); x2, y2, xy = central second moments; a, b, theta (degrees, in (-90, 90]) =
 *                   the moments' ellipse as SExtractor's A_IMAGE, B_IMAGE, THETA_IMAGE define it (a^2, b^2 =
 *                   (x2 + y2)/2 +- sqrt(((x2 - y2)/2)^2 + xy^2), tan 2 theta = 2 xy / (x2 - y2)); peak =
 *                   max w at (xpeak, ypeak), the first maximum in raster order
 *   out_flags_i32 : int32 [nlabels]: bit 0 the segment touches the frame border, bit 1 flux <= 0 (x, y,
 *                   moments and ellipse are NaN), bit 2 a masked or non-finite pixel lies inside the box
 * All sums are float64 in a fixed order: results are bit-identical from run to run.
 */
#define SPX_MEASURE_COLUMNS 13
int spx_measure_labels_f32(const float* frame, const uint8_t* bad_mask, double bkg_scalar, const float* bkg_map,
                           const int32_t* labels, int fny, int fnx, int nlabels, const int32_t* boxes,
                           double* out_table_f64, int32_t* out_flags_i32, void* stream);
int spx_measure_labels_f64(const double* frame, const uint8_t* bad_mask, double bkg_scalar, const double* bkg_map,
                           const int32_t* labels, int fny, int fnx, int nlabels, const int32_t* boxes,
                           double* out_table_f64, int32_t* out_flags_i32, void* stream);

/*
 * Per-source error measurements of labels 1..nlabels: flux error, the covariance of the flux-weighted centre
 * and a FWHM, the columns the reference's catalogue carries beside the positions (catalogs.py: fluxerr, fwhm ->
 * pos_std -> weight) and align.find_linear_fit(use_weights=True) fits with.
 *   frame, bad_mask, bkg_scalar, bkg_map, labels, fny, fnx, nlabels, boxes : as given to spx_measure_labels_*
 *   table_f64 : the table spx_measure_labels_* wrote for the same labels; flux, x, y and peak are taken from its
 *               row, so both calls agree on them to the bit
 *   rms_map   : the noise per pixel in the frame's dtype (spx_background_maps_*'s rms), or NULL: rms_scalar
 *   gain      : electrons per data unit; > 0 and finite adds the source's own Poisson noise, else none
 * A pixel p of label l inside its box is usable when v_p is finite, p is not masked and labels[p] == l.  Over
 * the usable pixels, in float64:
 *     w_p  = v_p - bkg_p
 *     s_p  = rms at p; an s_p that is not finite or < 0 counts as 0 and raises SPX_EFLAG_NOISE
 *     v2_p = s_p * s_p + (w_p / gain if gain > 0 and finite and w_p > 0, else 0)
 *   out_errors_f64 : float64 [nlabels][SPX_ERROR_COLUMNS], row l - 1 = (fluxerr, errx2, erry2, errxy, nhalf, fwhm)
 *     fluxerr = sqrt(sum v2_p)                                 (SExtractor's FLUXERR_ISO, restated)
 *     errx2 = sum(v2_p ux^2) / flux^2, erry2 = sum(v2_p uy^2) / flux^2, errxy = sum(v2_p ux uy) / flux^2 with
 *             ux = x_p - x, uy = y_p - y: the first-order variance of the flux-weighted centre, since
 *             d x / d I_p = (x_p - x) / flux; all three NaN unless the table's flux is > 0 and finite
 *     nhalf = the number of usable pixels with w_p >= 0.5 peak (an exact count; 0 unless peak > 0)
 *     fwhm  = 2 sqrt(nhalf / pi), the diameter of the circle whose area is the half-maximum area (NaN unless
 *             peak > 0)
 *   out_eflags_i32 : int32 [nlabels], values that continue spx_measure_labels_*'s flags: SPX_EFLAG_HALFMAX when
 *             the label has usable pixels and all of them lie above half maximum (nhalf == npix: fwhm is a lower
 *             bound), SPX_EFLAG_NOISE as above
 * All sums are float64 in a fixed order: results are bit-identical from run to run and independent of the grid.
 * SPX_E_ARG: nlabels < 0, or a null frame, labels, boxes, table or output; SPX_E_SHAPE: fny or fnx < 1, or
 * fny * fnx >= 2^31 - 1; both before any HIP call.  nlabels == 0 succeeds and writes nothing.
 */
#define SPX_ERROR_COLUMNS 6
#define SPX_EFLAG_HALFMAX 32
#define SPX_EFLAG_NOISE 64
int spx_measure_errors_f32(const float* frame, const uint8_t* bad_mask, double bkg_scalar, const float* bkg_map,
                           double rms_scalar, const float* rms_map, double gain, const int32_t* labels, int fny,
                           int fnx, int nlabels, const int32_t* boxes, const double* table_f64,
                           double* out_errors_f64, int32_t* out_eflags_i32, void* stream);
int spx_measure_errors_f64(const double* frame, const uint8_t* bad_mask, double bkg_scalar, const double* bkg_map,
                           double rms_scalar, const double* rms_map, double gain, const int32_t* labels, int fny,
                           int fnx, int nlabels, const int32_t* boxes, const double* table_f64,
                           double* out_errors_f64, int32_t* out_eflags_i32, void* stream);

/*
 * Deblending of merged sources: a multi-threshold tree per segment of a label image and a level-by-level
 * flood from the branches that count, in the spirit of SExtractor's DEBLEND_NTHRESH / DEBLEND_MINCONT.  The
 * definition is this library's own (SExtractor's tree is unpinned); after two IEEE steps per pixel it is
 * integer arithmetic throughout, so labels are bit-reproducible and independent of scheduling, grid size and
 * of whether a parent's state lived in LDS or in the workspace.
 *   frame, bad_mask, filter, fky, fkx, fny, fnx : as spx_detect_label_*.  f is the filtered image as defined
 *       there (same fused multiply-add chain in the frame's dtype; v' = 0 outside the frame and at masked or
 *       non-finite pixels; without a filter f = v'), converted exactly to float64
 *   labels   : int32 [fny][fnx], labels 1..nlabels (others count as background)
 *   boxes    : int32 [nlabels + 1][4], the table spx_label_bboxes_i32 writes (row = label)
 *   nlevels  : n with n + 1 in {2, 4, 8, 16, 32, 64};  contrast : c in [0, 1];  mode : 0 exponential, 1 linear
 * Per parent P (the pixels of one label inside its box; other labels inside the box are ignored everywhere):
 *  1. lo = min f, hi = max f over P.  hi <= lo: the parent is left whole.
 *     q(p) = min(2^30, floor(((f(p) - lo) / (hi - lo)) * 2^30)), an integer; float64, every operation rounded
 *     on its own.  F(X) = sum of q over X, an exact 64-bit integer.
 *  2. TQ_0 = 0.  Mode 0 with lo > 0 and rho = hi / lo finite: g = rho with sqrt applied log2(n + 1) times,
 *     p_0 = 1, p_k = p_(k-1) * g, x_k = ((p_k - 1) / (rho - 1)) * 2^30, TQ_k = min(2^30, ceil(x_k)), k = 1..n.
 *     Mode 1, and every other case of mode 0: TQ_k = k * 2^30 / (n + 1).  All float64, each step rounded on
 *     its own, only + - * / sqrt.  S_k = {p in P : q(p) >= TQ_k}; S_0 = P.
 *  3. Tree, k = n down to 0.  The children of a connected component C of S_k (`connectivity`) are the
 *     components of S_(k+1) inside C.  A child D is significant when objs(D) is not empty, or when
 *     (double)F(D) >= c * (double)F(P) and |D| >= min_area.  With two or more significant children objs(C) is
 *     the union over the significant children of objs(D) if that is not empty, else {D}.  Otherwise objs(C) is
 *     the (at most one) non-empty objs(D) among its children, or empty; then C as a whole goes on as one
 *     candidate, its insignificant bumps included.  objs(P) empty: the parent is left whole.  Otherwise the
 *     members of objs(P) are the seeds, numbered 1..m in raster order of each seed's first pixel.
 *  4. Flood.  o(p) = the seed number on seed pixels, 0 elsewhere.  For k = n down to 0, synchronous sweeps
 *     until one changes nothing: every p in P with o(p) = 0 and q(p) >= TQ_k that has a neighbour
 *     (`connectivity`) with o > 0 in the PREVIOUS sweep's state takes the o of the neighbour with the largest q;
 *     ties go to the smallest o.  All of a connected P ends up assigned (pixels of a parent that is not
 *     connected under `connectivity` and that no seed can reach stay together as one further child).
 *  5. Parents whose bounding box holds more than SPX_DEBLEND_MAX_BOX_PIXELS pixels are left whole and flagged.
 *   work       : spx_deblend_workspace_bytes(fny, fnx, nlabels) bytes of device memory (0 for sizes the call
 *                refuses); too small or NULL: SPX_E_WORKSPACE, and nothing is written
 *   out_labels : int32 [fny][fnx] (not `labels` itself): every final segment, children and untouched parents,
 *                numbered 1..L' in raster order of its first pixel
 *   out_parent : int32 [max_out], row l' - 1 = the input label the segment came from
 *   out_dflags : int32 [max_out], bit 3 (8) the segment is a child of a split parent, bit 4 (16) the parent
 *                was over the box limit and was not examined; the values continue spx_measure_labels_*'s flags
 *   max_out    : rows of out_parent / out_dflags; rows beyond are not written and out_nlabels still holds the
 *                true count.  fny * fnx / min_area rows suffice for labels made with the same min_area
 *   out_nlabels: int32 [1] on the DEVICE: L', or -1 if a union-find chain failed its consistency check
 * SPX_E_ARG: null pointer (bad_mask and filter may be NULL), connectivity not 4 / 8, min_area < 1, nlabels or
 * max_out < 0, nlevels + 1 not a power of two in 2..64, contrast outside [0, 1] or NaN, mode not 0 / 1, even
 * filter side or side > 7; SPX_E_SHAPE: fny or fnx < 1, or fny * fnx >= 2^31 - 1.  All checked before any HIP call.
 */
#define SPX_DEBLEND_MAX_BOX_PIXELS 65536
#define SPX_FLAG_DEBLENDED 8
#define SPX_FLAG_NODEBLEND 16
size_t spx_deblend_workspace_bytes(int fny, int fnx, int nlabels);
int spx_deblend_labels_f32(const float* frame, const uint8_t* bad_mask, const float* filter, int fky, int fkx,
                           int fny, int fnx, const int32_t* labels, int nlabels, const int32_t* boxes,
                           int connectivity, int min_area, int nlevels, double contrast, int mode, void* work,
                           size_t work_bytes, int32_t* out_labels, int32_t* out_parent, int32_t* out_dflags,
                           int max_out, int32_t* out_nlabels, void* stream);
int spx_deblend_labels_f64(const double* frame, const uint8_t* bad_mask, const double* filter, int fky, int fkx,
                           int fny, int fnx, const int32_t* labels, int nlabels, const int32_t* boxes,
                           int connectivity, int min_area, int nlevels, double contrast, int mode, void* work,
                           size_t work_bytes, int32_t* out_labels, int32_t* out_parent, int32_t* out_dflags,
                           int max_out, int32_t* out_nlabels, void* stream);

/*
 * Sky background and noise maps (the background mesh SExtractor starts with; the reference gets both maps
 * from it): frame -> per-cell sigma-clipped statistics -> median-filtered mesh -> bicubic-spline maps, and the
 * detection threshold map spx_detect_label_* takes.  The definitions are this library's own.
 *
 * MESH.  Cells of bh x bw pixels; ncy = ceil(fny / bh), ncx = ceil(fnx / bw); the last cell of an axis may be
 * partial.  8 <= bh, bw <= 128 and bh * bw <= 16384 (float64 frames: 8192), so that a cell's values fit 64 KiB
 * of LDS: anything else is SPX_E_SHAPE.  float64 frames are processed in float64, float32 frames in float32.
 * USABLE PIXEL: finite, bad_mask (uint8, non-zero = bad, or NULL) clear, and labels (int32 segmentation of an
 * earlier spx_detect_label_*, or NULL) zero.
 * PER CELL, on the n usable values sorted ascending, with the range [lo, hi) = [0, n):
 *   1. med = median of sorted[lo:hi]; an even count takes (a + b) * 0.5 of the two middle values in float64.
 *   2. If sorted[lo] == sorted[hi - 1] (all values equal): mean = that value, std = 0, stop.  Otherwise mean and
 *      std (population standard deviation, two passes) in float64 with a fixed reduction order.
 *   3. Stop if std is not > 0 or max_iters rounds are done (max_iters = 0: no clipping).
 *   4. The new range is the part of [lo, hi) with med - kappa std <= v <= med + kappa std (contiguous in the
 *      sorted values: two binary searches).  Stop if it equals the old range, or if it would be empty (only
 *      possible for kappa < 1; the old range is kept); otherwise go to 1.
 *   mesh_rms = std;  mesh_bkg = mean if std == 0, 2.5 med - 1.5 mean if |mean - med| < 0.3 std, else med;
 *   mesh_ngood = n (the count before clipping).  A cell is BAD when n < max(2, ceil(min_good_fraction *
 *   cell_pixels)), cell_pixels being the true pixel count of a partial cell: its mesh_bkg and mesh_rms are NaN.
 *   SPX_E_ARG: null frame or output, kappa not positive and finite, max_iters < 0, min_good_fraction outside
 *   0..1.  Results are bit-identical from run to run.
 * MAPS.  A mesh cell counts as good when mesh_ngood >= 2 and neither mesh value is NaN (what
 * spx_background_mesh_* writes; a caller may knock further cells out the same way).
 *   Filter, for the bkg and the rms mesh alike, filter_size fs in {1, 3, 5, 7} (else SPX_E_ARG): every cell, good
 *   or bad, takes the median of the good cells in the fs x fs window around it, truncated at the mesh border
 *   (even count: mean of the two middle values; fs = 1: good cells keep their value).  A window without a
 *   good cell takes the median of all good cells of the mesh.  A mesh without any good cell sets bit 0 of
 *   `status` (int32 on the device, written by every call) and the maps are NaN.
 *   Expansion: tensor-product natural cubic spline through the filtered mesh, knots at the uniform cell
 *   centres cy_j = j bh + (bh - 1) / 2, cx_i = i bw + (bw - 1) / 2 (also for a partial last cell); pixel
 *   coordinates outside [c_0, c_last] are clamped to it; one knot on an axis: constant along it, two: linear.
 *   This is scipy.interpolate.CubicSpline(bc_type='natural') along y, then along x, evaluated in float64 and
 *   rounded once to the maps' dtype; rms_out is clamped at 0 from below first.
 *   thr_out = float32(double(bkg as stored) + nsigma * double(rms as stored)), the threshold frame of
 *   spx_detect_label_*.  Each of bkg_out, rms_out, thr_out may be NULL (all three: SPX_E_ARG).
 *   work: spx_background_workspace_bytes(fny, fnx, bh, bw) bytes (0 for sizes the calls refuse); too small or
 *   NULL: SPX_E_WORKSPACE.  It starts with float64 planes [2][6][ncy * ncx]: plane [0][0] is the filtered
 *   background mesh, plane [1][0] the filtered rms mesh, the others spline coefficients.
 *   SPX_E_SHAPE: frame or box sizes as above, or ncy, ncx not ceil(fny / bh), ceil(fnx / bw).
 */
size_t spx_background_workspace_bytes(int fny, int fnx, int bh, int bw);
int spx_background_mesh_f32(const float* frame, const uint8_t* bad_mask, const int32_t* labels, int fny, int fnx,
                            int bh, int bw, double kappa, int max_iters, double min_good_fraction,
                            double* mesh_bkg, double* mesh_rms, int32_t* mesh_ngood, void* stream);
int spx_background_mesh_f64(const double* frame, const uint8_t* bad_mask, const int32_t* labels, int fny, int fnx,
                            int bh, int bw, double kappa, int max_iters, double min_good_fraction,
                            double* mesh_bkg, double* mesh_rms, int32_t* mesh_ngood, void* stream);
int spx_background_maps_f32(const double* mesh_bkg, const double* mesh_rms, const int32_t* mesh_ngood, int ncy,
                            int ncx, int bh, int bw, int filter_size, int fny, int fnx, double nsigma, void* work,
                            size_t work_bytes, float* bkg_out, float* rms_out, float* thr_out, int32_t* status,
                            void* stream);
int spx_background_maps_f64(const double* mesh_bkg, const double* mesh_rms, const int32_t* mesh_ngood, int ncy,
                            int ncx, int bh, int bw, int filter_size, int fny, int fnx, double nsigma, void* work,
                            size_t work_bytes, double* bkg_out, double* rms_out, float* thr_out, int32_t* status,
                            void* stream);

/*
 * Half-pixel dithered blots: for every source the four images image00, image10, image01,
 * image11 that spx_find_displacement5_f32 takes (align.py:664-676), resampled from the
 * source's drizzled cutout with the separable quintic ('poly5') interpolant.
 *   src    : float32 [nbatch][sny][snx] drizzled cutouts (masked pixels already 0), sny, snx >= 6
 *   affine : float64 [nbatch][6] = (a0..a5): target pixel (x', y') (0-based, un-dithered grid)
 *            lies at source pixel (a0 x' + a1 y' + a2, a3 x' + a4 y' + a5)
 *   gain   : float32 [nbatch] factor applied to the samples (blot.py:134-150: exposure-time /
 *            pixel-area scaling), or NULL for 1
 *   im4    : float32 [nbatch][4][ny][nx]; dither (ox, oy) in {0, 1/2}^2 (imct.dx -= ox,
 *            imct.dy -= oy) samples target position (x + ox, y + oy) (cutout.py:1138: cutout
 *            pixel x lies at image position x + blc - dx); points mapping outside the source are 0.
 */
int spx_blot_affine4_f32(const float* src, int64_t nbatch, int sny, int snx, const double* affine,
                         const float* gain, int ny, int nx, float* im4, void* stream);

/*
 * The same four blots through a map that is NOT affine over the cutout (instrument distortion:
 * what the reference's BlotWCSMap evaluates per pixel, blot.py:21-76): per source a bivariate
 * polynomial of total degree `degree` (1..5) in the target position relative to the cutout centre,
 *   u = x + ox - (nx-1)/2,  v = y + oy - (ny-1)/2,
 *   xs = sum_{d=0..degree} sum_{i=d..0} coef[b][0][k] u^i v^(d-i),  k = d(d+1)/2 + (d-i),
 *   ys likewise with coef[b][1][k];
 *   coef : float64 [nbatch][2][21] (21 slots per axis whatever the degree; unused ones ignored).
 * subpixal_amd.blot.poly_from_map fits the coefficients from any callable map and reports the
 * residual; everything else as spx_blot_affine4_f32.  Parity with drizzlepac: UNPINNED.
 */
int spx_blot_poly4_f32(const float* src, int64_t nbatch, int sny, int snx, const double* coef,
                       int degree, const float* gain, int ny, int nx, float* im4, void* stream);

/*
 * Catalog-scale entries (round 3): the body of the loop align.py:656-699 for a whole catalog whose cutouts
 * all have DIFFERENT shapes (bounding box + padding per source, cutout.py:159-175), without a host loop
 * over sources or pixels.  Packed layout shared by the three calls: item p's (h x w) pixels, row-major, at
 * element item_offset[p] of a flat float32 buffer; its four dithered blots at 4 * item_offset[p]
 * (order 00, 10, 01, 11); its interlaced image (2h x 2w) at 4 * item_offset[p] of `out_icc`;
 * item_shape = int32 [nbatch][2] = (h, w).  Each call has a float64 sibling (`_f64`, the blots
 * `_to_f64`) for catalogs of float64 frames: the reference computes in the cutouts' dtype.
 */

/* frame -> packed cutouts (cutout.py:689-797 slicing/fill + align.py:661 zeroing; see spx_gather_cutouts_f32
 * for `fill`, `fmask`, `seg`, `ids`): boxes int32 [nbatch][4] = (x0, y0, w, h). */
int spx_gather_cutouts_var_f32(const float* frame, const uint8_t* fmask, int fny, int fnx,
                               const int32_t* boxes, int64_t nbatch, const int64_t* item_offset,
                               float fill, float* packed, const int32_t* seg, const int32_t* ids,
                               void* stream);
/* ... for a float64 frame: frame, fill and packed are float64 (the packed layout of the float64 catalog) */
int spx_gather_cutouts_var_f64(const double* frame, const uint8_t* fmask, int fny, int fnx,
                               const int32_t* boxes, int64_t nbatch, const int64_t* item_offset,
                               double fill, double* packed, const int32_t* seg, const int32_t* ids,
                               void* stream);

/* packed drizzled cutouts -> packed blots (the four blot_cutout calls of align.py:664-676 per source).
 *   map    : degree == 0: float64 [nbatch][6] affine maps as spx_blot_affine4_f32;
 *            degree 1..5: float64 [nbatch][2][21] polynomial maps as spx_blot_poly4_f32
 *   src_*  : layout of the drizzled cutouts, dst_* : layout of the image cutouts the blots are made for
 *            (sources smaller than 6 px per side give all-zero blots) */
int spx_blot4_var_f32(const float* src, const int64_t* src_offset, const int32_t* src_shape,
                      int64_t nbatch, const double* map, int degree, const float* gain,
                      const int64_t* dst_offset, const int32_t* dst_shape, float* im4, void* stream);
/* ... with the blots stored as float64, for float64 image cutouts (blot.py:155 writes tblot's float32
 * result into a copy of the image cutout): src, the resampling and gain stay float32 (blot.py:134), so each
 * value is spx_blot4_var_f32's, widened exactly. */
int spx_blot4_var_to_f64(const float* src, const int64_t* src_offset, const int32_t* src_shape,
                         int64_t nbatch, const double* map, int degree, const float* gain,
                         const int64_t* dst_offset, const int32_t* dst_shape, double* im4, void* stream);

/* cc.find_displacement for every item of a packed catalog: ONE call launches each kernel family named in
 * `family_mask` (bit 0: larger side 3..32 px, bit 1: 33..64, bit 2: 65..85, bit 3: 86..128) over the same
 * tables; each family takes its own items and leaves the others alone.  Items no launched family takes
 * (a side below 3 or above 128 px, or a family whose bit is not set) are NOT written: pre-fill out_dxdy /
 * out_status with your "not measured" values.  workspace: spx_workspace_bytes_xcorr(nbatch, 128, 128)
 * bytes when bit 3 is set, else none.  out_icc must be given. */
#define SPX_FAMILY_32 1
#define SPX_FAMILY_64 2
#define SPX_FAMILY_85 4
#define SPX_FAMILY_128 8
int spx_find_displacement5_catalog_f32(const float* ref, const float* im4, const int64_t* item_offset,
                                       const int32_t* item_shape, int64_t nbatch, int family_mask,
                                       int cc_type, double* out_dxdy, int32_t* out_status,
                                       float* out_icc, void* workspace, size_t workspace_bytes,
                                       void* stream);
/* ... for float64 cutouts and blots (the packed float64 catalog): masks, statistics and normalisation in
 * float64 before the float32 transforms, as spx_find_displacement5_f64; out_icc stays float32. */
int spx_find_displacement5_catalog_f64(const double* ref, const double* im4, const int64_t* item_offset,
                                       const int32_t* item_shape, int64_t nbatch, int family_mask,
                                       int cc_type, double* out_dxdy, int32_t* out_status,
                                       float* out_icc, void* workspace, size_t workspace_bytes,
                                       void* stream);

/*
 * Drizzle: the forward resampler of dithered frames onto one output grid, for affine maps (what the reference's
 * resample.py gets from drizzlepac; drizzlepac is not in the reference tree, so parity with it is UNPINNED.  The
 * definition is this library's own, after Fruchter & Hook 2002, PASP 114, 144; tests/drizzle_statement.py restates
 * it in numpy as a scatter and the kernel is pinned against that).
 *
 * DEFINITION
 *   Coordinates: pixels are 0-based, pixel (i, j) has its centre at integer coordinates and covers
 *   [i - 1/2, i + 1/2] x [j - 1/2, j + 1/2] (the blot's convention).
 *   Inputs, for frames k = 0 .. K-1 (1 <= K <= 128): data D_k [ny_k][nx_k], all frames in one dtype (float32 or
 *   float64), shapes may differ; an optional weight map W_k >= 0 of the same dtype (none: weight 1); an optional
 *   uint8 bad-pixel mask; a forward affine map from input to output pixels,
 *       (X, Y) = (a0 x + a1 y + a2, a3 x + a4 y + a5),  float64 [6]  (the layout of blot.shift_affine)
 *   with det A != 0 (a negative determinant, a mirrored frame, is allowed); an `active` flag.
 *   An input pixel has effective weight 0 when it is masked, its value is not finite, its weight is not finite, or
 *   its weight is <= 0.
 *   Drop: the drop of pixel (i, j) is the square of side pixfrac p in (0, 1] centred on it.
 *   kernel 0 'square': Q is the parallelogram M_k(drop); a = area(Q n P_XY) / (|det A| p^2), the fraction of the
 *                      drop that lands on output pixel P_XY.
 *   kernel 1 'turbo' : Q is replaced by the axis-aligned square of side p sqrt|det A| centred on M_k(i, j); a is the
 *                      overlap over that square's area.
 *   kernel 2 'point' : a = 1 for the pixel (floor(X + 1/2), floor(Y + 1/2)) that holds M_k(i, j), 0 elsewhere.
 *   An overlap area below 1e-12 output pixels^2 counts as 0 (rounding noise of a drop that only touches the pixel).
 *   Accumulation: num = sum a w d and wht = sum a w over active frames in ascending k, then j ascending, then i
 *   ascending; everything float64 with contraction off.  sci = num / wht where wht > 0, else `fill`; sci is written
 *   in the frame dtype, wht as float32.  ctx is int32 planes [ceil(K / 32)][NY][NX]: bit k % 32 of plane k / 32 is
 *   set iff frame k added a w > 0 to that pixel.
 *   sci is a weighted mean of input values, i.e. input-pixel surface brightness: NO scale^2 is applied.
 *   Geometry is float64 throughout.  Frames and the output hold fewer than 2^31 - 1 pixels each.
 *   The result does not depend on scheduling or the grid: one thread owns one output pixel and sums in the order
 *   above (a gather; there are no atomics).
 *
 * Two steps.  spx_drizzle_rows is a HOST function: it checks the frames' description and packs one row of
 * SPX_DRIZZLE_ROW_BYTES per frame (pointers, shape, flag, the map, its inverse, the candidate window and the drop's
 * edge vectors and slopes, all computed once in float64) into out_rows, a HOST buffer of
 * nframes * SPX_DRIZZLE_ROW_BYTES.  The caller copies the rows to the device and keeps them there; changing one
 * frame's map or flag rewrites one row.  spx_drizzle_f32 / _f64 take that DEVICE table and only launch, so they
 * can be captured and never copy behind the caller's back.
 *
 * spx_drizzle_rows -- every array is a HOST array; the pointers inside frames / weights / masks are device pointers
 *   frames   : [nframes] frame pointers (none may be NULL)
 *   weights  : [nframes] weight-map pointers; the table or single entries may be NULL (weight 1)
 *   masks    : [nframes] uint8 mask pointers; the table or single entries may be NULL
 *   shapes   : int32 [nframes][2] = (ny, nx)
 *   maps_f64 : float64 [nframes][6]
 *   active   : uint8 [nframes], or NULL: every frame is active
 *   pixfrac, kernel (SPX_DRIZZLE_SQUARE / _TURBO / _POINT), out_ny, out_nx: as above; rows depend on pixfrac and
 *   kernel, so pass the same kernel to spx_drizzle_*
 *   SPX_E_ARG: nframes outside 1 .. 128, pixfrac outside (0, 1] or not finite, unknown kernel, a null table or frame,
 *   a map with an entry that is not finite, a singular map.  SPX_E_SHAPE: a frame or the output with a side < 1 or
 *   2^31 - 1 pixels or more; a map under which one output pixel would gather from more than 8 x 8 input pixels
 *   (2 rx + 1 > 8 for the window's half-side rx: at pixfrac 1 a frame shrunk more than sixfold).  On an error nothing is written.
 *
 * spx_drizzle_f32 / _f64
 *   rows     : the DEVICE copy of what spx_drizzle_rows packed, [nframes] rows
 *   fill     : sci where no drop lands
 *   out_sci  : [out_ny][out_nx] in the frame dtype;  out_wht : float32 [out_ny][out_nx]
 *   out_ctx  : int32 [ceil(nframes / 32)][out_ny][out_nx]
 *   SPX_E_ARG: nframes, kernel, null pointer; SPX_E_SHAPE: output size.  Checked before any HIP call.
 */
#define SPX_DRIZZLE_ROW_BYTES 224
#define SPX_DRIZZLE_SQUARE 0
#define SPX_DRIZZLE_TURBO 1
#define SPX_DRIZZLE_POINT 2
int spx_drizzle_rows(const void* const* frames, const void* const* weights, const uint8_t* const* masks,
                     const int32_t* shapes, const double* maps_f64, const uint8_t* active, int nframes,
                     double pixfrac, int kernel, int out_ny, int out_nx, void* out_rows);
int spx_drizzle_f32(const void* rows, int nframes, int kernel, double fill, int out_ny, int out_nx, float* out_sci,
                    float* out_wht, int32_t* out_ctx, void* stream);
int spx_drizzle_f64(const void* rows, int nframes, int kernel, double fill, int out_ny, int out_nx, double* out_sci,
                    float* out_wht, int32_t* out_ctx, void* stream);

/*
 * Drizzle for frames with polynomial distortion maps: spx_drizzle_poly_rows, spx_drizzle_poly_f32 / _f64.
 *
 * DEFINITION.  Everything of the drizzle above that is not named here is unchanged: pixel convention, effective
 * weight, accumulation order (k, then j, then i ascending), float64 with contraction off, sci = num / wht, fill, ctx,
 * the 1e-12 px^2 drop threshold, and no scale^2 applied.
 *   Map of frame k: a bivariate polynomial of total degree `degree` (1 .. 5) in the input position relative to a
 *   per-frame centre (xc, yc):  u = x - xc, v = y - yc,
 *       X = sum_{d=0..degree} sum_{i=d..0} coef[0][k] u^i v^(d-i),   k = d (d + 1) / 2 + (d - i),
 *       Y likewise with coef[1][k];
 *   coef is float64 [2][21]: the term order and the 21 slots of spx_blot_poly4_f32; slots above `degree` are ignored.
 *   Evaluation order.  spx_drizzle_poly_rows re-expands the map about the frame's own centre
 *   (xf, yf) = ((nx - 1) / 2, (ny - 1) / 2) in extended precision and rounds each coefficient once, so the centre a
 *   map is given about does not matter to the result.  A position is (u, v) = ((i - xf) +- p/2, (j - yf) +- p/2) and
 *   the value a nested Horner scheme, powers of v outside and of u inside:
 *       acc = c(0, D);  for j = D-1 .. 0 { r = c(D-j, j); for i = D-j-1 .. 0: r = r u + c(i, j);  acc = acc v + r }
 *   (c(i, j) the coefficient of u^i v^j; D (D + 3) / 2 multiply-add pairs).  A computed coordinate is within
 *   (4 D + 3) eps sum |c(i, j) u^i v^j| of the polynomial's value: 2 D roundings on the longest path through the
 *   scheme, D ulps of the sum for the rounding of u and as many for v, 1 for the coefficients, 2 to spare.
 *   kernel 0 'square': Q is the quadrilateral with straight edges whose vertices are M applied to the four corners
 *                      (i -+ p/2, j -+ p/2) of the drop, in that cyclic order; a = area(Q n P_XY) / area(Q), both
 *                      areas absolute values (a mirrored map comes out right).  For a degree-1 map this is the affine
 *                      definition (area(Q) = |det A| p^2).
 *   kernel 1 'turbo' : the axis-aligned square of side s = p sqrt|det J(i, j)| centred on M(i, j), J the analytic
 *                      Jacobian of M at the pixel centre; a = overlap / (s s).
 *   kernel 2 'point' : a = 1 on the pixel that holds M(i, j).
 *
 * spx_drizzle_poly_rows -- the sibling of spx_drizzle_rows: every array is a HOST array
 *   frames, weights, masks, shapes, active, pixfrac, kernel, out_ny, out_nx: as for spx_drizzle_rows
 *   coef_f64   : float64 [nframes][2][21]
 *   degree     : int32 [nframes], 1 .. 5 (an affine frame is a degree-1 row)
 *   center_f64 : float64 [nframes][2] = (xc, yc)
 *   out_rows   : HOST buffer of nframes * SPX_DRIZZLE_POLY_ROW_BYTES.  A row's first 40 bytes are laid out as the
 *                affine row's (data, weight and mask pointers, ny, nx, active, reserved); then the re-expanded
 *                coefficients, the frame's centre, the inverse of the Jacobian at that centre and the number of chord
 *                iterations (the kernel's inverse estimate), the candidate window (rx, ry), the reach of the linear
 *                estimate (the tile skip) and the bounds of a drop's bounding half-sides over the whole frame, all
 *                computed once in float64.  csrc/spx_drizzle_poly_kernels.h says why no drop with a non-zero overlap
 *                can fall outside the window.
 *   SPX_E_ARG: as spx_drizzle_rows, and: a degree outside 1 .. 5; a used coefficient or a centre that is not finite;
 *   a map whose Jacobian determinant is zero, not finite or of both signs over the frame, checked on a lattice of
 *   33 x 33 positions evenly spaced from -1/2 to nx - 1/2 and -1/2 to ny - 1/2 (the frame's border, corners and
 *   centre among them).  SPX_E_SHAPE: as spx_drizzle_rows; a map under which some output pixel would gather from
 *   more than 8 x 8 input pixels anywhere in the frame (2 rx + 1 > 8), or whose Jacobian varies by half or more of
 *   itself over the frame (no window can be given).  On an error nothing is written.
 *
 * spx_drizzle_poly_f32 / _f64 -- take the DEVICE copy of those rows and only launch: capturable, no hidden copies.
 *   Arguments, outputs and errors exactly as spx_drizzle_f32 / _f64, checked before any HIP call.
 */
#define SPX_DRIZZLE_POLY_ROW_BYTES 488
int spx_drizzle_poly_rows(const void* const* frames, const void* const* weights, const uint8_t* const* masks,
                          const int32_t* shapes, const double* coef_f64, const int32_t* degree,
                          const double* center_f64, const uint8_t* active, int nframes, double pixfrac, int kernel,
                          int out_ny, int out_nx, void* out_rows);
int spx_drizzle_poly_f32(const void* rows, int nframes, int kernel, double fill, int out_ny, int out_nx, float* out_sci,
                         float* out_wht, int32_t* out_ctx, void* stream);
int spx_drizzle_poly_f64(const void* rows, int nframes, int kernel, double fill, int out_ny, int out_nx,
                         double* out_sci, float* out_wht, int32_t* out_ctx, void* stream);

/*
 * Cosmic-ray rejection for the drizzle: the steps the reference's Resample.execute runs between its two drizzles
 * (resample.py:366-390: median, blot back, derivative, drizCR).  drizzlepac is not in the reference tree, so, as for
 * the drizzle itself, parity with it is UNPINNED: the definition is this library's own, modelled on drizzlepac's
 * createMedian / ablot / quickDeriv / drizCR; tests/crreject_statement.py restates steps 2 .. 6 in numpy and the
 * kernels are pinned against that (step 1 is the drizzle's own arithmetic, pinned by tests/drizzle_statement.py).
 *
 * DEFINITION -- notation of the drizzle above: frames k with rows, maps M_k, effective weights, pixfrac, a kernel.
 *   1. Single-frame values.  For output pixel P and active frame k, num_k and wht_k are the drizzle's sums
 *      restricted to frame k, in the same order, float64, contraction off.  s_k = (float)(num_k / wht_k), valid iff
 *      wht_k > 0.  For float32 frames this is bit for bit what spx_drizzle_f32 writes with only frame k active.
 *   2. Median.  m = the number of valid frames at P; nmed = m (uint8).  The m values are sorted ascending; if
 *      m - nlow - nhigh >= 1 the nlow lowest and the nhigh highest are dropped, otherwise none.  med is the middle
 *      value, for an even count (float)(0.5 * ((double)a + (double)b)) of the two middle values; med = 0 where
 *      m = 0.  med is float32 for both frame dtypes.
 *   3. Blot.  For input pixel (i, j) of frame k, (X, Y) = M_k(i, j) = ((a0 i + a1 j) + a2, (a3 i + a4 j) + a5) and
 *      b(i, j) = the quintic of spx_blot_affine4_f32 (with its edge continuation) of med at (X, Y), float32.  With
 *      ix = floor(X), iy = floor(Y), b is DEFINED iff 0 <= X <= NX-1 and 0 <= Y <= NY-1 and every med pixel of the
 *      footprint [ix-2, ix+3] x [iy-2, iy+3], clipped to the grid, has nmed > 0.  b is also evaluated at positions
 *      (i, j) outside the frame: the map is defined there.
 *   4. Derivative.  D(i, j) = the largest |b(i, j) - b(n)| over those of the four neighbours n = (i+-1, j),
 *      (i, j+-1) whose b is defined; 0 if none is.  float32.
 *   5. Test.  A pixel is TESTABLE iff it lies inside the frame, its value is finite, it is not masked, its weight
 *      (where a weight map is given) is finite and > 0, b is defined there, and its rms is finite and >= 0.  In
 *      float64 with contraction off: t = |d - b|, var = rms^2 + (max(b - sky, 0) / gain if gain is finite and > 0,
 *      else 0), fail_p = testable and t > scale_p * D + snr_p * sqrt(var), p = 1, 2.  rms is a per-frame scalar or a
 *      map in the frame's dtype.  Pixels that are not testable never fail.
 *   6. Mask.  crmask(i, j) = fail_2(i, j) and (some pixel of the 3 x 3 block around (i, j) has fail_1).
 *      clean(i, j) = b cast to the frame dtype where crmask is 1; elsewhere d, unchanged, NaNs included.
 *   drizzlepac's defaults: snr = (3.5, 3.0), scale = (1.2, 0.7), nlow = nhigh = 0, sky = 0, no gain.
 *
 * Two or three frames (spx_drizzle_minmed_*, spx_drizzle_cr_grow_*).  With K = 2 the median is the mean and carries
 * half of every hit, with K = 3 it carries every pixel that two frames are hit at; steps 2' and 7 are what
 * drizzlepac answers that with (combine_type = 'minmed', combine_grow; driz_cr_grow, driz_cr_ctegrow).  They are
 * modelled on drizzlepac, which is not in the reference tree: parity with it is UNPINNED here too, the definition is
 * this library's own and tests/minmed_statement.py restates it in numpy.  Every decision below is float64 with
 * contraction off and uses + - * / and comparisons only (no sqrt), so numpy reproduces it to the bit.
 *   2'. minmed, in place of step 2.  For output pixel P with m valid s_k:
 *      md   = step 2's value, with nlow / nhigh as given;  lo = the smallest valid s_k (0 where m = 0);
 *      kmin = the lowest table row among the frames that supplied lo;
 *      var  = r^2 + (g > 0 ? max((double)lo - sky, 0) / g : 0) with (r, sky, g) = row kmin of the table
 *             (combine_rms, sky, gain) [nframes][3];
 *      t    = (double)md - (double)lo;
 *      hit_p = m >= 2 and t > 0 and t t > (n_p n_p) var, for (n_1, n_2) = nsigma, n_2 <= n_1;  seed = hit_1;
 *      use_min = seed or (hit_2 and some pixel within Chebyshev distance `grow` of P, inside the grid, is a seed);
 *      med = use_min ? lo : md;  nmed = m as before;
 *      minmed (uint8) = 0 median, 1 minimum by the pixel's own test, 2 minimum by the neighbour rule.
 *      grow = 0: no neighbour rule.
 *   7. Growth of the mask, after step 6.  Seeds are step 6's crmask.  A pixel that is not a seed becomes flagged
 *      iff it is TESTABLE in step 5's sense (inside the frame, finite, unmasked, weight > 0, valid rms, b defined)
 *      and a seed lies in the g x g block centred on it (g odd, 1 .. 9) or at (i, j - ctedir tau) for some
 *      tau = 1 .. c (c = ctegrow 0 .. 64, ctedir -1, 0 or +1: the readout tail runs along the frame's columns).
 *      The grown crmask = seed or flagged.  For a newly flagged pixel clean = (T)b, the same b step 5 compares with
 *      (the same operations in the same order); every other pixel of clean stays as step 6 left it.
 *      g = 1 together with c = 0 or ctedir = 0: no step 7.
 *   Not here: the other combine types, static masks.  The frames are taken as they are: a caller whose frames
 *   differ in sky level subtracts it first (spx_sky_stats_* below).
 *
 * Both entries take the DEVICE table spx_drizzle_rows packed and only launch, as spx_drizzle_* do; neither has an
 * atomic or depends on the grid, so every output is the same bit pattern on every run.  They can be captured, with
 * one exception: the first spx_drizzle_median_* call on a device with nactive > 64 (more than 64 KiB of LDS) raises the
 * kernel's dynamic-LDS limit before it launches, so make that call once outside a capture; later calls only launch.
 *
 * spx_drizzle_median_f32 / _f64 -- steps 1 and 2 over the rows' own masks
 *   nactive  : the number of rows whose `active` flag is set (the caller counts them when it packs the rows); the
 *              launch takes nactive * 1024 bytes of LDS per workgroup.  Values of active rows beyond that count
 *              would be dropped.
 *   kernel   : the kernel the rows were packed for;  nlow, nhigh >= 0
 *   out_med  : float32 [out_ny][out_nx];  out_nmed : uint8 [out_ny][out_nx]
 *   SPX_E_ARG: a null pointer, nframes outside 1 .. 128, nactive outside 1 .. nframes, unknown kernel, nlow or nhigh
 *   < 0.  SPX_E_SHAPE: output size as for spx_drizzle_*.  Checked before any HIP call.
 *
 * spx_drizzle_cr_f32 / _f64 -- steps 3 .. 6 for row `frame` of the table (its data, weight, mask, shape and map)
 *   fny, fnx : the frame's shape; they size the grid only, the kernel addresses by the row's own ny, nx
 *   med, nmed: what spx_drizzle_median_* wrote for the (out_ny, out_nx) grid, at least 6 x 6 (the quintic's edge
 *              continuation)
 *   rms_scalar, rms_map : the frame's noise, a scalar, or (rms_map not NULL) a map of the frame's shape and dtype
 *   sky, gain: of step 5; a gain that is not finite or not > 0 switches the Poisson term off; sky must be finite
 *   out_crmask : uint8 [ny][nx];  out_clean : [ny][nx] in the frame dtype; it must not be the frame itself
 *   SPX_E_ARG: a null pointer (rms_map may be NULL), nframes outside 1 .. 128, frame outside 0 .. nframes-1, an snr
 *   or scale that is not finite or < 0, snr2 > snr1, scale2 > scale1, a sky that is not finite.  SPX_E_SHAPE: a
 *   frame or output with a side < 1 or 2^31 - 1 pixels or more, an output below 6 x 6.  Checked before any HIP call.
 */
int spx_drizzle_median_f32(const void* rows, int nframes, int nactive, int kernel, int nlow, int nhigh, int out_ny,
                           int out_nx, float* out_med, uint8_t* out_nmed, void* stream);
int spx_drizzle_median_f64(const void* rows, int nframes, int nactive, int kernel, int nlow, int nhigh, int out_ny,
                           int out_nx, float* out_med, uint8_t* out_nmed, void* stream);
int spx_drizzle_cr_f32(const void* rows, int nframes, int frame, int fny, int fnx, const float* med,
                       const uint8_t* nmed, int out_ny, int out_nx, double rms_scalar, const float* rms_map, double sky,
                       double gain, double snr1, double snr2, double scale1, double scale2, uint8_t* out_crmask,
                       float* out_clean, void* stream);
int spx_drizzle_cr_f64(const void* rows, int nframes, int frame, int fny, int fnx, const float* med,
                       const uint8_t* nmed, int out_ny, int out_nx, double rms_scalar, const double* rms_map,
                       double sky, double gain, double snr1, double snr2, double scale1, double scale2,
                       uint8_t* out_crmask, double* out_clean, void* stream);

/*
 * spx_drizzle_minmed_f32 / _f64 -- steps 1, 2 and 2' in two launches: the median's gather, which also writes lo and
 * the two decision bits, and a 32 x 8 stencil pass with a halo of `grow` for the neighbour rule.  It takes the place
 * of spx_drizzle_median_* (arguments rows .. nhigh, out_med, out_nmed and the LDS note as there; the same exception
 * for a capture when nactive > 64).  Neither pass reads a plane it writes.
 *   table_f64 : DEVICE float64 [nframes][3] = (combine_rms, sky, gain) per table row; a gain that is not > 0 (0, NaN):
 *              no Poisson term.  It cannot be checked without a copy: the caller gives finite rms >= 0 and sky.
 *   nsigma1, nsigma2 : n_1 >= n_2 >= 0;  grow : 0 .. 8
 *   out_md, out_lo : float32 [out_ny][out_nx], step 2's median and the minimum;  out_bits : uint8, hit_1 | hit_2 << 1
 *   out_med, out_nmed, out_minmed : the results of step 2'
 *   SPX_E_ARG: a null pointer, nframes outside 1 .. 128, nactive outside 1 .. nframes, unknown kernel, nlow or nhigh
 *   < 0, an nsigma that is not finite or < 0, nsigma2 > nsigma1, grow outside 0 .. 8, out_med the same plane as out_md
 *   or out_lo, out_minmed the same as out_bits or out_nmed, out_bits the same as out_nmed.  SPX_E_SHAPE: output size as
 *   for spx_drizzle_*.  Checked before any HIP call.
 *
 * spx_drizzle_cr_grow_f32 / _f64 -- step 7 for row `frame`, one launch after spx_drizzle_cr_* (arguments rows .. out_nx,
 * rms_scalar and rms_map as there)
 *   seed     : uint8 [ny][nx], what spx_drizzle_cr_* wrote as out_crmask
 *   grow, ctegrow, ctedir : g odd 1 .. 9, c 0 .. 64, -1 | 0 | +1
 *   out_crmask : uint8 [ny][nx], the grown mask; it must not be `seed`
 *   clean    : [ny][nx] in the frame dtype, what spx_drizzle_cr_* wrote as out_clean; only newly flagged pixels are
 *              written
 *   SPX_E_ARG: a null pointer (rms_map may be NULL), nframes outside 1 .. 128, frame outside 0 .. nframes-1, grow even
 *   or outside 1 .. 9, ctegrow outside 0 .. 64, ctedir outside -1 .. 1, out_crmask == seed.  SPX_E_SHAPE: as for
 *   spx_drizzle_cr_*.  Checked before any HIP call.
 */
int spx_drizzle_minmed_f32(const void* rows, int nframes, int nactive, int kernel, int nlow, int nhigh,
                           const double* table_f64, double nsigma1, double nsigma2, int grow, int out_ny, int out_nx,
                           float* out_md, float* out_lo, uint8_t* out_bits, float* out_med, uint8_t* out_nmed,
                           uint8_t* out_minmed, void* stream);
int spx_drizzle_minmed_f64(const void* rows, int nframes, int nactive, int kernel, int nlow, int nhigh,
                           const double* table_f64, double nsigma1, double nsigma2, int grow, int out_ny, int out_nx,
                           float* out_md, float* out_lo, uint8_t* out_bits, float* out_med, uint8_t* out_nmed,
                           uint8_t* out_minmed, void* stream);
int spx_drizzle_cr_grow_f32(const void* rows, int nframes, int frame, int fny, int fnx, const float* med,
                            const uint8_t* nmed, int out_ny, int out_nx, double rms_scalar, const float* rms_map,
                            const uint8_t* seed, int grow, int ctegrow, int ctedir, uint8_t* out_crmask,
                            float* clean, void* stream);
int spx_drizzle_cr_grow_f64(const void* rows, int nframes, int frame, int fny, int fnx, const float* med,
                            const uint8_t* nmed, int out_ny, int out_nx, double rms_scalar, const double* rms_map,
                            const uint8_t* seed, int grow, int ctegrow, int ctedir, uint8_t* out_crmask,
                            double* clean, void* stream);

/*
 * Sigma-clipped statistics of WHOLE frames: the sky level that resample.DeviceDrizzle (skysub=True) subtracts from
 * each frame before the drizzle, where the reference runs sky.subtractSky (resample.py:359-364).  The library's own
 * definition, in the spirit of drizzlepac's skystat / skyclip / skylsigma / skyusigma / skylower / skyupper;
 * drizzlepac is not in the reference tree, so parity with it is UNPINNED, as for the rest of the drizzle.  It is the
 * mesh-cell rule of spx_background_mesh_* (steps 1-4 there) over all usable pixels of a frame, with separate lower
 * and upper clip factors and optional hard bounds.
 *
 * A pixel is USABLE when its value is finite, its mask byte is 0 (or there is no mask), its weight (where a weight
 * map is given) is finite and > 0, and lower <= v <= upper for each bound that is given (a NaN bound: none).
 * n_usable is their count.  The closed range [lo, hi] starts at the hard bounds (-inf / +inf where there is none).
 * Rounds r = 0 .. max_iters:
 *   1. n = the count of usable values in [lo, hi].  n == 0: stop, status SPX_SKY_EMPTY; sky, med, mean and std are
 *      NaN (possible only in round 0).
 *   2. med = the exact median of those values (even count: (a + b) * 0.5 of the two middle values, in float64).
 *   3. min == max over those values: mean = that value, std = 0, stop.  Otherwise, in float64 with contraction off,
 *      S1 = sum(v - med), S2 = sum((v - med)^2), mean = med + S1 / n, std = sqrt(max(S2 / n - (S1 / n)^2, 0)).
 *      THE ORDER OF THE TWO SUMS IS FIXED and does not depend on the device, its CU count or on scheduling: number
 *      the frame's pixels i = y * nx + x.  4096 accumulators j = 0 .. 4095, each starting from 0.0, add the terms
 *      of the pixels j, j + 4096, j + 8192, ... in that order (pixels outside the range are skipped).  Accumulators
 *      64 g .. 64 g + 63 are then added by a butterfly: for m = 32, 16, 8, 4, 2, 1 every accumulator becomes
 *      itself + its partner (index ^ m); the 64 results g = 0 .. 63 are added four at a time in order of g starting
 *      from 0.0 (0.0 + s_4q + s_4q+1 + s_4q+2 + s_4q+3, q = 0 .. 15), and these 16 in order of q starting from 0.0.
 *   4. Stop if std is not > 0 or r == max_iters.
 *   5. lo' = max(lo, med - lsigma * std), hi' = min(hi, med + usigma * std), each product and sum rounded on its own.
 *      If the count inside [lo', hi'] equals n: stop.  If it is 0 (factors < 1): keep the old range and stop.
 *      Otherwise [lo, hi] = [lo', hi'] and go to 1.
 * Results per frame: med, mean, std, lo, hi of the last round whose statistics were computed, n_usable, n_final = n of
 * that round, rounds = the number of rounds whose statistics were computed, status, and
 *   sky = med (SPX_SKY_MEDIAN), mean (SPX_SKY_MEAN), or for SPX_SKY_MODE the mesh rule: mean if std == 0,
 *   2.5 med - 1.5 mean if |mean - med| < 0.3 std, else med.
 * -0.0 counts as +0.0; the sign of a zero result is not part of the definition.
 *
 * The median is found by radix selection over the order-preserving integer image of the values (integer histograms:
 * exact and independent of scheduling), so every result is the same bit pattern on every run and every device.
 *
 * spx_sky_stats_f32 / _f64 -- all frames in one launch sequence; the call only enqueues (one memset and
 * (max_iters + 1) (2 D + 2) + 2 kernels, D = 3 / 6 digits for float32 / float64), copies nothing to the host and can
 * be captured.  Each frame is read (max_iters + 1) (D + 1) times at most; a frame that has stopped is not read again.
 *   frames, weights, masks : DEVICE arrays of nframes device pointers (frames in the call's dtype, weights in the
 *              same dtype, masks uint8, nonzero = bad), each frame row-major [ny][nx] and contiguous.  weights and
 *              masks may be NULL as a whole, and each of their entries may be NULL.
 *   shapes   : DEVICE int32 [nframes][2] = (ny, nx).  A frame with a side < 1, 2^31 - 1 pixels or more, or a NULL
 *              frame pointer gets status SPX_SKY_BAD_FRAME and NaN statistics: shapes cannot be checked without a copy.
 *   lower, upper : hard bounds, NaN = none;  lsigma, usigma : clip factors;  max_iters : clipping rounds after round 0
 *   stat     : SPX_SKY_MEDIAN, SPX_SKY_MEAN or SPX_SKY_MODE
 *   work     : spx_sky_workspace_bytes(nframes) bytes (0 for nframes outside 1 .. 128), 8-byte aligned; too small or
 *              NULL: SPX_E_WORKSPACE
 *   out      : float64 [nframes][6] = sky, med, mean, std, lo, hi
 *   out_counts : int64 [nframes][2] = n_usable, n_final;  out_status : int32 [nframes][2] = status bits, rounds
 *   SPX_E_ARG: a null table (frames, shapes) or output, nframes outside 1 .. 128, lsigma or usigma not positive and
 *   finite, max_iters < 0 or > 1000, unknown stat, lower > upper.  Everything is checked before any HIP call.
 */
#define SPX_SKY_MEDIAN 0
#define SPX_SKY_MEAN 1
#define SPX_SKY_MODE 2
#define SPX_SKY_EMPTY 1     /* status bit: no usable pixel */
#define SPX_SKY_BAD_FRAME 2 /* status bit: a side < 1, too many pixels, or a NULL frame */
size_t spx_sky_workspace_bytes(int nframes);
int spx_sky_stats_f32(const void* const* frames, const void* const* weights, const uint8_t* const* masks,
                      const int32_t* shapes, int nframes, double lower, double upper, double lsigma, double usigma,
                      int max_iters, int stat, void* work, size_t work_bytes, double* out, int64_t* out_counts,
                      int32_t* out_status, void* stream);
int spx_sky_stats_f64(const void* const* frames, const void* const* weights, const uint8_t* const* masks,
                      const int32_t* shapes, int nframes, double lower, double upper, double lsigma, double usigma,
                      int max_iters, int stat, void* work, size_t work_bytes, double* out, int64_t* out_counts,
                      int32_t* out_status, void* stream);

/*
 * Synthetic Gaussian-spot pairs: pair k = first_index + i has
 * tx, ty ~ U(-max_shift, max_shift), sigma ~ U(sigma_lo, sigma_hi), amplitude ~
 * U(0.5, 2) from a counter-based generator keyed by (seed, k); ref has the spot
 * at the tile centre, img at centre + (tx, ty).  truth_dxdy float64 [nbatch][2]
 * (may be NULL).
 */
int spx_gen_gaussian_pairs_f32(uint64_t seed, int64_t first_index, int64_t nbatch, int n,
                               float sigma_lo, float sigma_hi, float max_shift, float* ref,
                               float* img, double* truth_dxdy, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SUBPIXAL_HIP_H */
