"""The host-side plumbing the seams share: what is a torch tensor, which context and stream a call runs on, numpy <-> torch dtypes, and the
way an array gets onto a device and back.  Without torch the module still imports: the host memspace works without it."""

import numpy as np

from ._lib import MEM_DEVICE, MEM_HOST, default_context

try:
    import torch
except ImportError:  # pragma: no cover
    torch = None

DEVICE = "cuda:0"  # where a numpy input is worked on when the caller names no device
_DEVICE_INDEX = int(DEVICE.rpartition(":")[2])


def is_torch(a):
    return a is not None and type(a).__module__.startswith("torch")


def bound_context(dev=None, ctx=None):
    """``ctx`` (without one: the default context of ``dev``, a ``torch.device``, a string or None for ``DEVICE``) with torch's current
    stream of the context's own device set on it.  Of ``ctx`` only ``.device`` and ``.set_stream`` are used.  This runs before every
    launch: the device is named to torch by its index, the form torch resolves soonest, and nothing is built per call."""
    if ctx is None:
        ctx = default_context(_DEVICE_INDEX if dev is None else (dev if isinstance(dev, torch.device) else torch.device(dev)).index or 0)
    ctx.set_stream(torch.cuda.current_stream(ctx.device).cuda_stream)
    return ctx


def device_of(*arrays, device=None):
    """The device of the first CUDA tensor among ``arrays``, else ``device`` (None: ``DEVICE``)."""
    for a in arrays:
        if is_torch(a) and a.is_cuda:
            return a.device
    return torch.device(device or DEVICE)


def np_dtype(a):
    """The numpy dtype of a tensor's or an array's elements."""
    return np.dtype(str(a.dtype).replace("torch.", "")) if is_torch(a) else np.asarray(a).dtype


def torch_dtype(dtype):
    return getattr(torch, np.dtype(dtype).name)


def compare_value(threshold, dtype):
    """The float64 value of ``threshold`` after the rounding numpy applies to it in ``array_of_dtype >= threshold``: a Python float and a
    scalar of the array's type take the array's type, a wider numpy scalar promotes the comparison (and float32 -> float64 is exact)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.asarray(threshold).astype(np.result_type(dtype, threshold)))


def staged(a, dev, dtypes=None, label="{name}", layout="contiguous", astype=None):
    """A tensor on ``dev`` with the values of ``a``, a numpy array (of any byte order) or a torch tensor.  ``dtypes``: the numpy dtypes or
    their names that are accepted; another one raises ``TypeError(label.format(dtype=a.dtype, name=its numpy name))``.  ``layout``:
    "contiguous"; "rows": unit stride along the rows is enough; "any": a tensor keeps its strides.  A tensor that already is on ``dev``
    in that layout comes back as it is.  ``astype``: a numpy dtype the values are converted to (after the check of ``dtypes``)."""
    if not is_torch(a):
        a = np.asarray(a)
        if not a.dtype.isnative:  # (a FITS array is big-endian)
            a = a.astype(a.dtype.newbyteorder("="))
    if dtypes is not None:
        name = str(a.dtype).replace("torch.", "") if is_torch(a) else a.dtype.name  # (not every torch dtype has a numpy one)
        if name not in [np.dtype(d).name for d in dtypes]:
            raise TypeError(label.format(dtype=a.dtype, name=name))
    if is_torch(a):
        t = a.to(dev) if astype is None else a.to(dev, torch_dtype(astype))
    else:
        a = np.ascontiguousarray(a, dtype=astype)
        if a.dtype == np.uint16:  # (torch moves uint16 as bytes of the same layout)
            return torch.as_tensor(a.view(np.int16)).to(dev).view(torch.uint16)
        return torch.as_tensor(a).to(dev)
    if layout == "contiguous" or (layout == "rows" and t.numel() and t.stride(-1) != 1):
        t = t.contiguous()
    return t


def to_host(a):
    return a.detach().cpu().numpy() if is_torch(a) else np.asarray(a)


def out_array(shape, dtype, device):
    """(array, memspace, context): an empty torch tensor on ``device`` and its bound context, or a numpy array when ``device`` is None."""
    if device is None:
        return np.empty(shape, dtype=dtype), MEM_HOST, default_context()
    dev = torch.device(device)
    return torch.empty(shape, dtype=torch_dtype(dtype), device=dev), MEM_DEVICE, bound_context(dev)
