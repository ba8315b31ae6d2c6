"""Bright-object masks of the destripe set-up on the device: ``apply_object_mask`` of ``pyimcom.imdestripe`` (reference
src/pyimcom/imdestripe.py:781-872) and what ``Sca_img.__init__`` does with it (317-332).  The binding (seam 11):

    pyimcom.imdestripe.apply_object_mask = pyimcom_amd.objmask.apply_object_mask
    eng.add_sca(image, mask, g_eff, object_mask=(threshold_m, threshold_c, type))      # pyimcom_amd.destripe.DestripeEngine

The reference takes ``np.median`` of the whole image, a threshold and a 5 x 5 ``binary_dilation``; for ``type="jwst"`` three rounds of
sigma-clipped median / MAD, ``binary_propagation`` of the bright seeds through the fainter pixels and two more dilations.  csrc/objmask.hip
has the parts: an exact k-th order statistic (radix select; the MAD's ``|v - bkg|`` is formed on the fly), threshold and clipping flags,
the constrained propagation and the box dilation.  Their results are booleans, counts and order statistics, so they equal numpy's and
scipy's bit for bit.  scipy is not imported.

What stays on the host, in numpy scalars of the very types the reference has there, so that the promotion rules are numpy's own:
``threshold_m * median_val + threshold_c``, ``1.4826 * mad``, ``3.0 * sigma``, the two ``max(...)``, the ``sigma <= 0`` and
``count < 100`` breaks and ``not np.isfinite(sigma)``; the device receives each threshold as the value numpy would compare with.  The
``np.std(clip_vals)`` fallback (846), reached only when the MAD is 0, downloads the kept values and calls numpy: a pairwise float sum is
not worth reproducing on the device.

A numpy image gives numpy results (the mask as ``bool``); a torch tensor on a device gives tensors on that device (the mask as
``torch.bool``) and the image never visits the host.  Nothing here has been timed on a device yet (tools/bench_objmask.py)."""

import ctypes as C

import numpy as np

from ._dev import DEVICE, bound_context, compare_value, device_of, is_torch, np_dtype, staged  # noqa: F401 (DEVICE: a public name here)
from ._lib import MEM_DEVICE, ImcomError, check, lib, ptr

__all__ = ["apply_object_mask", "object_mask", "median", "order_statistics", "propagate", "dilate", "jwst_valid", "setup_bytes", "DILATE_TILE",
           "PROPAGATE_TILE", "DILATE_MAX_R"]

DILATE_TILE = (32, 48)  # rows, columns of output pixels of a dilation workgroup (csrc/objmask.hip)
PROPAGATE_TILE = 62  # side of a propagation tile
DILATE_MAX_R = 8
IMCOM_ERR_UNSUPPORTED = -4
_WORKSPACE = 64 << 10  # the selection's state and histograms, rounded up


def _image(a, dev):
    """A contiguous float32 / float64 tensor on ``dev`` with the values of ``a``."""
    return staged(a, dev, (np.float32, np.float64), "objmask: a float32 or float64 image, not {dtype}")


def _flags(a, dev, shape=None):
    """A contiguous uint8 tensor on ``dev``: a bool / uint8 tensor as it is, anything else as ``!= 0``."""
    import torch

    if not is_torch(a):
        a = np.asarray(a)
        a = a if a.dtype == np.bool_ else a != 0
    t = staged(a, dev, layout="any")
    t = t.view(torch.uint8) if t.dtype == torch.bool else t if t.dtype == torch.uint8 else (t != 0).view(torch.uint8)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"objmask: flags of shape {tuple(t.shape)} for an array of shape {tuple(shape)}")
    return t.contiguous()


# ---- the kernels' callers: tensors on one device in, tensors out ----
def _select(ctx, t, flags=None, k=-1, center=None):
    """(value k, value k + 1, m, NaNs) among the flagged elements of ``t`` (``k`` < 0: the two middle ones); with ``center`` of |t - center|."""
    import torch

    out = torch.empty(2, dtype=t.dtype, device=t.device)
    info = torch.empty(2, dtype=torch.int64, device=t.device)
    check(lib.imcom_select_kth(ctx.handle, ptr(t), int(t.dtype == torch.float64), t.numel(), ptr(flags), int(center is not None),
                               float(center) if center is not None else 0.0, int(k), ptr(out), ptr(info), MEM_DEVICE))
    v, i = out.cpu().numpy(), info.cpu().numpy()
    return v[0], v[1], int(i[0]), int(i[1])


def _median(ctx, t, flags=None, center=None):
    """``np.median`` of the flagged elements (of |t - center|): a numpy scalar of the array's type; NaN if any is NaN or none is flagged."""
    lo, hi, m, nans = _select(ctx, t, flags, -1, center)
    if m == 0 or nans:
        return lo.dtype.type(np.nan)
    with np.errstate(over="ignore"):
        return np.mean(np.array([lo, hi] if m % 2 == 0 else [lo], dtype=lo.dtype))  # numpy's own mean of the middle: one add and a halving


def _threshold(ctx, t, bkg, t_seed, t_grow=None, finite_only=True):
    import torch

    seed = torch.empty(t.shape, dtype=torch.uint8, device=t.device)
    grow = torch.empty_like(seed) if t_grow is not None else None
    dt = np_dtype(t)
    check(lib.imcom_mask_threshold(ctx.handle, ptr(t), int(t.dtype == torch.float64), t.numel(), float(bkg), compare_value(t_seed, dt),
                                   compare_value(t_grow, dt) if t_grow is not None else 0.0, int(finite_only), ptr(seed), ptr(grow), MEM_DEVICE))
    return seed, grow


def _clip(ctx, t, keep_in=None, bkg=0.0, limit=0.0):
    """(flags, count): ``isfinite(t)`` without ``keep_in``, else ``keep_in & (|t - bkg| < limit)``."""
    import torch

    keep = torch.empty(t.shape, dtype=torch.uint8, device=t.device)
    count = torch.empty(1, dtype=torch.int64, device=t.device)
    check(lib.imcom_mask_clip(ctx.handle, ptr(t), int(t.dtype == torch.float64), t.numel(), ptr(keep_in), float(bkg), compare_value(limit, np_dtype(t)),
                              ptr(keep), ptr(count), MEM_DEVICE))
    return keep, int(count.item())


def _propagate(ctx, seed, grow):
    import torch

    out = torch.empty_like(seed)
    sweeps = C.c_long(0)
    check(lib.imcom_mask_propagate(ctx.handle, ptr(seed), ptr(grow), int(seed.shape[0]), int(seed.shape[1]), ptr(out), C.byref(sweeps), MEM_DEVICE))
    return out, sweeps.value


def _dilate(ctx, mask, r):
    import torch

    out = torch.empty_like(mask)
    check(lib.imcom_mask_dilate(ctx.handle, ptr(mask), int(mask.shape[0]), int(mask.shape[1]), int(r), ptr(out), MEM_DEVICE))
    return out


def _apply(ctx, src, mask, dst):
    import torch

    code = {torch.float32: 0, torch.float64: 1, torch.uint8: 2}[src.dtype]
    check(lib.imcom_mask_apply(ctx.handle, ptr(src), code, ptr(mask), src.numel(), ptr(dst), MEM_DEVICE))
    return dst


# ---- public helpers ----
def _result(t, like, as_bool=True):
    import torch

    if is_torch(like):
        return t.view(torch.bool) if as_bool and t.dtype == torch.uint8 else t
    a = t.cpu().numpy()
    return a.view(np.bool_) if as_bool and a.dtype == np.uint8 else a


def order_statistics(a, k, where=None, device=None):
    """(k-th smallest, (k + 1)-th smallest or the largest) of ``a`` (of its elements where ``where``), as ``np.partition`` places them;
    NaNs sort last.  numpy scalars of the array's type."""
    dev = device_of(a, where, device=device)
    t = _image(a, dev)
    f = None if where is None else _flags(where, dev, t.shape)
    if not 0 <= int(k) < t.numel():  # (the entry reads a negative rank as "the middle" and refuses one past the array)
        raise ValueError(f"objmask: rank {k} of {t.numel()} values")
    lo, hi, m, _ = _select(bound_context(dev), t, f, int(k))
    if int(k) >= m:  # fewer flagged than the rank asks for
        raise ValueError(f"objmask: rank {k} of {m} values")
    return lo, hi


def median(a, where=None, center=None, device=None):
    """``np.median(a)`` or ``np.median(a[where])`` for a float32 / float64 array or tensor of any shape: exact, a numpy scalar of the
    array's type.  Any NaN among the values gives NaN, as numpy does; so does an empty selection.  With ``center`` the median of
    ``np.abs(a - center)``, the differences formed in the array's type on the fly."""
    dev = device_of(a, where, device=device)
    t = _image(a, dev)
    f = None if where is None else _flags(where, dev, t.shape)
    if t.numel() == 0:
        return np_dtype(t).type(np.nan)
    return _median(bound_context(dev), t, f, None if center is None else np_dtype(t).type(center))


def propagate(seed, grow, device=None, return_sweeps=False):
    """``scipy.ndimage.binary_propagation(seed, mask=grow)`` for 2-D images, default structure (4-connectivity), border 0.  With
    ``return_sweeps`` also the number of sweeps over the tiles that it took."""
    dev = device_of(seed, grow, device=device)
    s = _flags(seed, dev)
    g = _flags(grow, dev, s.shape)
    if s.dim() != 2 or s.numel() == 0:
        raise ValueError(f"objmask: a 2-D image, not shape {tuple(s.shape)}")
    out, sweeps = _propagate(bound_context(dev), s, g)
    return (_result(out, seed), sweeps) if return_sweeps else _result(out, seed)


def dilate(mask, r, device=None):
    """``scipy.ndimage.binary_dilation(mask, structure=np.ones((2 r + 1, 2 r + 1)))`` for a 2-D image, border 0; 1 <= r <= 8."""
    if not 1 <= int(r) <= DILATE_MAX_R:
        raise ImcomError(IMCOM_ERR_UNSUPPORTED, f"objmask: dilation radius {r}, served are 1 .. {DILATE_MAX_R}")
    dev = device_of(mask, device=device)
    m = _flags(mask, dev)
    if m.dim() != 2 or m.numel() == 0:
        raise ValueError(f"objmask: a 2-D image, not shape {tuple(m.shape)}")
    return _result(_dilate(bound_context(dev), m, r), mask)


def jwst_valid(image, mask=None):
    """``Sca_img.apply_jwst_mask`` (imdestripe.py:412-419): (the image with its NaNs set to 0, ``mask & ~isnan(image)``, or the valid
    pixels alone without a mask).  Two torch expressions for a tensor, the reference's numpy lines for an array."""
    if is_torch(image):
        import torch

        valid = ~torch.isnan(image)
        return torch.where(valid, image, torch.zeros((), dtype=image.dtype, device=image.device)), valid if mask is None else torch.logical_and(mask, valid)
    valid = ~np.isnan(image)
    return np.where(valid, image, 0.0), valid if mask is None else np.logical_and(mask, valid)


def setup_bytes(shape, dtype, type="fits"):
    """Device bytes at the peak of ``object_mask`` for one image: the image in its own type, the flag images that live together (2 for the
    plain route; 6 and the propagation's second image for ``jwst``) and the selection's workspace."""
    npix = int(np.prod(shape))
    return npix * np.dtype(dtype).itemsize + npix * (7 if type == "jwst" else 2) + _WORKSPACE


def object_mask(image, threshold_m=0, threshold_c=0.3, type="fits", details=None):
    """The ``neighbor_mask`` of ``apply_object_mask`` for a 2-D float32 / float64 tensor on a device: a uint8 tensor there.  ``details``, a
    dict, receives every intermediate (the scalars as the host formed them, the flag images as tensors)."""
    import torch

    if image.dim() != 2 or image.numel() == 0:
        raise ValueError(f"objmask: a 2-D image, not shape {tuple(image.shape)}")
    t = _image(image, image.device)
    ctx = bound_context(t.device)
    d = details if details is not None else {}
    if type == "jwst":
        keep, count = _clip(ctx, t)  # valid = isfinite(image)
        d["n_valid"] = count
        if count == 0:
            high = torch.zeros(t.shape, dtype=torch.uint8, device=t.device)
            d["seed_threshold"] = d["grow_threshold"] = 0.0
        else:
            rounds = 0
            for _ in range(3):
                bkg = _median(ctx, t, keep)
                mad = _median(ctx, t, keep, center=bkg)
                sigma = 1.4826 * mad
                if sigma <= 0:
                    break
                kept, n_kept = _clip(ctx, t, keep, bkg, 3.0 * sigma)
                if n_kept < 100:
                    break
                keep, count = kept, n_kept
                rounds += 1
            bkg = _median(ctx, t, keep)
            mad = _median(ctx, t, keep, center=bkg)
            sigma = 1.4826 * mad
            d["std_fallback"] = False
            if not np.isfinite(sigma) or sigma <= 0:
                d["std_fallback"] = True
                sigma = np.std(t.cpu().numpy()[keep.cpu().numpy().view(np.bool_)]) if count > 1 else 0.0
            seed_threshold = max(threshold_c, 6.0 * sigma)
            grow_threshold = max(0.5 * threshold_c, 2.5 * sigma)
            seed, grow = _threshold(ctx, t, bkg, seed_threshold, grow_threshold, finite_only=True)
            grown, sweeps = _propagate(ctx, seed, grow)
            high = _dilate(ctx, grown, 2)  # 3 x 3, twice
            d.update(rounds=rounds, n_clip=count, bkg=bkg, mad=mad, sigma=sigma, seed_threshold=seed_threshold, grow_threshold=grow_threshold, seed_mask=seed,
                     grow_candidates=grow, grown_mask=grown, sweeps=sweeps)
    else:
        median_val = _median(ctx, t)
        threshold = threshold_m * median_val + threshold_c
        high, _ = _threshold(ctx, t, 0.0, threshold, finite_only=False)
        d.update(median_val=median_val, threshold=threshold)
    d["high_value_mask"] = high
    return _dilate(ctx, high, 2)  # 5 x 5


def apply_object_mask(image, mask=None, threshold_m=0, threshold_c=0.3, inplace=False, type="fits", *, device=None, details=None):
    """``apply_object_mask`` of imdestripe.py:781-872, its signature, defaults and return ``(image_out, neighbor_mask)``.

    ``image``: 2-D, float32 or float64.  A numpy array is worked on ``device`` (default ``objmask.DEVICE``) and gives numpy results, the
    mask as bool; a torch tensor on a device gives tensors there, the mask as torch.bool.  A given ``mask`` (an array, or a tensor for a
    tensor image) is applied as it is, as in the reference.  ``type``: "jwst" takes the clipped-background, seed-and-grow route, anything
    else ("fits", "asdf") the plain threshold.  An image without a finite pixel gives an empty mask with "jwst".  The standard deviation
    the "jwst" route falls back to when the MAD is 0 is numpy's, on the downloaded kept pixels (module docstring)."""
    on_device = is_torch(image)
    if not on_device:
        if mask is not None and isinstance(mask, np.ndarray):  # 814-815: nothing to compute
            neighbor_mask = mask
        else:
            image = np.asarray(image) if not isinstance(image, np.ndarray) else image
            t = _image(image, device_of(device=device))
            neighbor_mask = object_mask(t, threshold_m, threshold_c, type, details).cpu().numpy().view(np.bool_)
        if inplace:
            image[neighbor_mask] = 0
            return image, neighbor_mask
        return np.where(neighbor_mask, 0, image), neighbor_mask
    import torch

    t = _image(image, device_of(image, device=device))
    if mask is not None and (is_torch(mask) or isinstance(mask, np.ndarray)):
        m = _flags(mask, t.device, t.shape)
    else:
        m = object_mask(t, threshold_m, threshold_c, type, details)
    ctx = bound_context(t.device)
    if inplace:
        _apply(ctx, t, m, t)
        if t.data_ptr() != image.data_ptr():  # a view that was not contiguous, or an image that lived elsewhere
            image.copy_(t)
        return image, m.view(torch.bool)
    return _apply(ctx, t, m, torch.empty_like(t)), m.view(torch.bool)
