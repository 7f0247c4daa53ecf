"""Sigma-clipped statistics of whole frames on the device: the sky level ``resample.DeviceDrizzle`` subtracts from
each frame (``skysub=True``), where the reference runs ``sky.subtractSky`` (subpixal/resample.py:359-364).

``frame_stats`` is one call of ``spx_sky_stats_f32`` / ``_f64`` (csrc/spx_sky_kernels.h) over all frames: an exact
median by radix selection, float64 moments in a fixed order, the clipping rounds on the device.
include/subpixal_hip.h carries the definition in full.  It is the library's own, in the spirit of drizzlepac's
``skystat`` / ``skyclip`` / ``skylsigma`` / ``skyusigma`` / ``skylower`` / ``skyupper``; drizzlepac is not in the
reference tree, so parity with it is UNPINNED.  Its ``'match'`` sky methods, the static mask and its histogram mode
are not here.
"""
import numpy as np

from . import _ffi

__all__ = ['frame_stats', 'SkyStats', 'STATS', 'EMPTY', 'BAD_FRAME', 'MAX_FRAMES']

STATS = _ffi.SKY_STATS
EMPTY, BAD_FRAME = _ffi.SKY_EMPTY, _ffi.SKY_BAD_FRAME
MAX_FRAMES = 128
_DTYPES = ('float32', 'float64')


class SkyStats(object):
    """numpy columns, one entry per frame: ``sky``, ``median``, ``mean``, ``std``, ``lo``, ``hi`` (float64),
    ``n_usable``, ``n_final`` (int64), ``rounds``, ``status`` (int32; bits ``EMPTY``, ``BAD_FRAME``)"""
    __slots__ = ('sky', 'median', 'mean', 'std', 'lo', 'hi', 'n_usable', 'n_final', 'rounds', 'status')

    def __init__(self, out, counts, status):
        self.sky, self.median, self.mean, self.std, self.lo, self.hi = (out[:, k].copy() for k in range(6))
        self.n_usable, self.n_final = counts[:, 0].copy(), counts[:, 1].copy()
        self.status, self.rounds = status[:, 0].copy(), status[:, 1].copy()

    def __len__(self):
        return len(self.sky)

    def __repr__(self):
        return 'SkyStats(sky=%r, std=%r, n_final=%r, rounds=%r, status=%r)' % (
            self.sky, self.std, self.n_final, self.rounds, self.status)


def _dtype_name(a):
    return str(a.dtype).replace('torch.', '')


def check_parameters(stat='median', lower=None, upper=None, clip=5, lsigma=4.0, usigma=4.0):
    """the ValueErrors of ``frame_stats`` and of ``DeviceDrizzle``'s ``sky*`` keywords; returns the normalised
    ``(stat, lower, upper, clip, lsigma, usigma)`` with NaN for a bound that is not given"""
    if stat not in STATS:
        raise ValueError("stat must be one of %s, got %r." % (sorted(STATS), stat))
    lower = float('nan') if lower is None else float(lower)
    upper = float('nan') if upper is None else float(upper)
    if lower > upper:
        raise ValueError("lower (%r) must not exceed upper (%r)." % (lower, upper))
    if int(clip) != clip or not 0 <= clip <= 1000:
        raise ValueError("clip must be an integer 0 .. 1000 (clipping rounds), got %r." % (clip,))
    lsigma, usigma = float(lsigma), float(usigma)
    if not (np.isfinite(lsigma) and lsigma > 0 and np.isfinite(usigma) and usigma > 0):
        raise ValueError("lsigma and usigma must be positive and finite, got %r and %r." % (lsigma, usigma))
    return stat, lower, upper, int(clip), lsigma, usigma


def check_frames(frames, weights, masks):
    """the ValueErrors of the frame lists; returns ``(frames, weights, masks, dtype name)`` as lists"""
    frames = list(frames)
    K = len(frames)
    if not 1 <= K <= MAX_FRAMES:
        raise ValueError("frames: 1 .. %d frames, got %d." % (MAX_FRAMES, K))
    weights = K * [None] if weights is None else list(weights)
    masks = K * [None] if masks is None else list(masks)
    if len(weights) != K or len(masks) != K:
        raise ValueError("weights, masks: one entry (or None) per frame.")
    dt = _dtype_name(frames[0])
    if dt not in _DTYPES:
        raise ValueError("frames: dtype must be float32 or float64, got %s." % dt)
    for k, f in enumerate(frames):
        if len(f.shape) != 2 or min(f.shape) < 1 or _dtype_name(f) != dt:
            raise ValueError("frames: frame %d must be 2-D, not empty and %s like frame 0." % (k, dt))
        for what, m in (('weight map', weights[k]), ('mask', masks[k])):
            if m is not None and tuple(m.shape) != tuple(f.shape):
                raise ValueError("the %s of frame %d has shape %s, the frame %s."
                                 % (what, k, tuple(m.shape), tuple(f.shape)))
    return frames, weights, masks, dt


def stats_resident(frames, weights, masks, dtype, stat, lower, upper, clip, lsigma, usigma):
    """``frame_stats`` over tensors that are on the device already (contiguous, ``dtype``; masks uint8); the
    parameters as ``check_parameters`` returns them.  Nothing is copied but the four small tables."""
    import torch
    from . import device
    device.init()
    lib = _ffi.load()
    K = len(frames)
    dev = frames[0].device

    def table(ts):
        return torch.from_numpy(np.array([0 if t is None else t.data_ptr() for t in ts], np.uint64).view(np.int64)
                                ).to(dev)
    ft = table(frames)
    wt = table(weights) if any(w is not None for w in weights) else None
    mt = table(masks) if any(m is not None for m in masks) else None
    shapes = torch.from_numpy(np.array([tuple(f.shape) for f in frames], np.int32)).to(dev)
    nbytes = lib.spx_sky_workspace_bytes(K)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty((K, 6), dtype=torch.float64, device=dev)
    counts = torch.empty((K, 2), dtype=torch.int64, device=dev)
    status = torch.empty((K, 2), dtype=torch.int32, device=dev)
    fn = lib.spx_sky_stats_f32 if dtype == 'float32' else lib.spx_sky_stats_f64
    rc = fn(ft.data_ptr(), device.ptr(wt) or None, device.ptr(mt) or None, shapes.data_ptr(), K, lower, upper, lsigma,
            usigma, clip, STATS[stat], work.data_ptr(), nbytes, out.data_ptr(), counts.data_ptr(), status.data_ptr(),
            device.stream_ptr())
    if rc == _ffi.E_ARG:
        raise ValueError(lib.spx_last_error().decode())
    _ffi.check(rc)
    return SkyStats(out.cpu().numpy(), counts.cpu().numpy(), status.cpu().numpy())


def frame_stats(frames, weights=None, masks=None, stat='median', lower=None, upper=None, clip=5, lsigma=4.0,
                usigma=4.0):
    """Sigma-clipped statistics of every frame, on the device.

    frames : sequence of 1 .. 128 2-D numpy arrays or tensors, all float32 or all float64; shapes may differ.
    weights, masks : None, or per frame None or a map of the frame's shape (mask: nonzero = bad; a pixel whose weight
        is not finite or <= 0 is not used).
    stat : ``'median'``, ``'mean'`` or ``'mode'`` (``2.5 median - 1.5 mean`` where mean and median are close, the
        rule of the background mesh): what ``sky`` holds.
    lower, upper : hard bounds on the values used, or None.
    clip : clipping rounds after the first (0: none);  lsigma, usigma : the clip factors below and above the median.

    Returns a :class:`SkyStats`.  A frame without a usable pixel has ``status & EMPTY`` and NaN statistics."""
    stat, lower, upper, clip, lsigma, usigma = check_parameters(stat, lower, upper, clip, lsigma, usigma)
    frames, weights, masks, dt = check_frames(frames, weights, masks)
    import torch
    from . import device
    tdt = torch.float32 if dt == 'float32' else torch.float64
    fr = [device.to_device(f, tdt) for f in frames]
    wt = [None if w is None else device.to_device(w, tdt) for w in weights]
    mk = []
    for m in masks:
        if m is not None and not isinstance(m, torch.Tensor):
            m = torch.from_numpy(np.ascontiguousarray(m))
        mk.append(None if m is None else device.to_device(m != 0, torch.uint8))
    return stats_resident(fr, wt, mk, dt, stat, lower, upper, clip, lsigma, usigma)
