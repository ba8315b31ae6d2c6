"""The I24 layer codec of ``pyimcom.compress`` on the device (reference src/pyimcom/compress/i24.py: ``I24Cube.to_mode`` 367-437,
``i24compress`` 443-478, ``i24decompress`` 481-514).  The binding (seam 14):

    data, overflow = pyimcom_amd.i24.i24compress(im, scheme, pars)                  # compressutils.py: CompressedOutput.compress_layer
    im = pyimcom_amd.i24.i24decompress(data, scheme, pars, overflow=overflow)        # CompressedOutput.decompress, every ReadFile
    cubes, overflows = pyimcom_amd.i24.compress_layers(frames, pars_list)            # a block's layers in one call
    frames = pyimcom_amd.i24.decompress_layers(cubes, pars_list, overflows)          # float32 [L, ny, nx] on the device

``compress_all_blocks`` runs the codec over every non-science layer of every block and every diagnostics reader decompresses what it
opens, in numpy on one core (``unpackbits`` / ``transpose`` / ``packbits`` / ``cumsum``).  Here a layer that sits on the device is coded
there (csrc/i24.hip) and crosses to the host as 1 to 3 bytes a pixel, and a compressed layer read from disk is decoded on the device
where ``noisespec.power_spectrum_2d``, ``reportstats.layer_percentiles`` and ``StreamingQuantiles.add`` take it as it is.  Every result
equals the reference's bit for bit.

Served is ``ALPHA`` absent or 1 (every use in the reference is linear); another value raises ``ImcomError`` (IMCOM_ERR_UNSUPPORTED): that
path goes through numpy's float32 ``power``.  Also refused (IMCOM_ERR_ARG): ``VMAX <= VMIN`` or either not finite, ``SOFTBIAS >= 2**24``,
``ny * nx >= 2**31``, an I24B cube whose first axis is not ``(BITKEEP + 7) // 8``, an overflow position outside the image.

The parameters are read as ``I24Cube.__init__`` reads them (316-339): ``float()``, ``int()``, ``bool()`` of what the dict or FITS header
holds, so the string ``"False"`` for ``DIFF`` / ``REORDER`` is true as it is there; ``BITKEEP`` given as ``>= 24`` or ``<= 0`` raises
``ValueError`` (332-333), absent it is 24.  A NaN pixel gets the code of ``VMIN`` and no overflow entry (numpy's cast on x86-64).

FITS, the ``CPRESS`` table, HDU names and the process pool stay the caller's; no astropy is imported."""

import ctypes as C

import numpy as np

from ._dev import DEVICE, bound_context, is_torch, np_dtype, staged, to_host
from ._lib import I24Pars, ImcomError, check, lib, ptr

__all__ = ["i24compress", "i24decompress", "compress_layers", "decompress_layers", "OverflowTable", "parse_pars", "check_pars", "tile_constants", "RECOGNIZED_SCHEMES"]

RECOGNIZED_SCHEMES = ["I24A", "I24B"]  # i24.py:36


def parse_pars(pars):
    """The parameters of one layer as ``I24Cube.__init__`` reads them (316-339), as an ``I24Pars`` record."""
    vmin, vmax = float(pars["VMIN"]), float(pars["VMAX"])
    softbias = int(pars["SOFTBIAS"]) if "SOFTBIAS" in pars else 0
    diff = bool(pars["DIFF"]) if "DIFF" in pars else False
    alpha = float(pars["ALPHA"]) if "ALPHA" in pars else 1.0
    if "BITKEEP" in pars:
        bitkeep = int(pars["BITKEEP"])
        if bitkeep >= 24 or bitkeep <= 0:
            raise ValueError(f"Can't keep {bitkeep:d} bits")
    else:
        bitkeep = 24
    reorder = bool(pars["REORDER"]) if "REORDER" in pars else True
    if softbias >= 2**24:  # (before the C long: any size of Python int)
        raise ImcomError(-1, f"i24: SOFTBIAS = {softbias}; served are 0 .. 2^24 - 1 and -1")
    return I24Pars(vmin, vmax, alpha, max(softbias, -2), bitkeep, int(diff), int(reorder))


def _records(pars_list):
    return (I24Pars * len(pars_list))(*[parse_pars(p) for p in pars_list])


def _sizes(recs, ny, nx, scheme):
    out = (C.c_long * 8)()
    check(lib.imcom_i24_sizes(len(recs), int(ny), int(nx), recs, RECOGNIZED_SCHEMES.index(scheme), out))
    return list(out)


def check_pars(pars_list, ny, nx, scheme="I24B"):
    """Raises what a call with these parameters and this shape would raise (no device is touched)."""
    _sizes(_records(list(pars_list)), ny, nx, scheme)


def tile_constants():
    """(pixels of a tile, tile sums a step of the scan of tile sums takes): csrc/i24_core.h's I24_TILE and I24_SCAN_CHUNK."""
    s = _sizes(_records([{"VMIN": 0.0, "VMAX": 1.0}]), 1, 1, "I24B")
    return int(s[5]), int(s[6])


class OverflowTable:
    """The overflow table of one layer (368-375): ``.data["y" | "x" | "value"]`` as ``I24Cube`` reads them (417-419); ``y`` and ``x`` int32
    (FITS format ``J``), ``value`` float32 (``E``), in ascending flat pixel order.  Device tensors when the layer was a device tensor."""

    def __init__(self, y, x, value):
        self.data = {"y": y, "x": x, "value": value}

    def __len__(self):
        return int(self.data["y"].shape[0])

    def columns(self):
        """The three host arrays, for ``fits.Column(name=..., format="J" | "J" | "E", array=...)``."""
        return tuple(to_host(v) for v in (self.data["y"], self.data["x"], self.data["value"]))


def _frames_view(frames, dev):
    """float32 [L, ny, nx] on the device with unit column stride and one layer stride, read in place when it already is that."""
    import torch

    if isinstance(frames, (list, tuple)):
        frames = torch.stack([staged(f, dev, layout="any") for f in frames])
    t = staged(frames, dev, layout="any")
    if t.dtype != torch.float32 or t.dim() != 3:
        raise TypeError(f"compress_layers: float32 [L, ny, nx], not {t.dtype} {tuple(t.shape)}")
    if t.numel() and not (t.stride(2) == 1 and t.stride(1) >= t.shape[2] and t.stride(0) >= 0):
        t = t.contiguous()
    return t


def compress_layers(frames, pars_list, scheme="I24B", ctx=None, device=None):
    """``i24compress`` of L layers with a parameter dict each, in one call.  frames: float32 [L, ny, nx], a device tensor (a crop of a
    larger one is read in place) or a numpy array (uploaded), or a list of 2-D ones.  Returns (cubes, overflows): per layer the uint8
    [nb, ny, nx] cube (I24B) or the int32 [ny, nx] image (I24A), views of one device tensor, and its ``OverflowTable`` on the device."""
    import torch

    if scheme not in RECOGNIZED_SCHEMES:
        raise ValueError(f"compress_layers: scheme {scheme!r} is none of {RECOGNIZED_SCHEMES}")
    dev = torch.device(device or DEVICE)
    pars_list = list(pars_list)
    recs = _records(pars_list)
    t = _frames_view(frames, dev)
    L, ny, nx = t.shape
    if L != len(pars_list):
        raise ValueError(f"compress_layers: {L} layers and {len(pars_list)} parameter dicts")
    sz = _sizes(recs, ny, nx, scheme)
    n = ny * nx
    if scheme == "I24A":
        out = torch.empty((L, ny, nx), dtype=torch.int32, device=dev)
    else:
        out = torch.empty((L, sz[3] // n, ny, nx), dtype=torch.uint8, device=dev)
    state = torch.empty(sz[0] // 4, dtype=torch.int32, device=dev)
    counts = (C.c_long * L)()
    ctx = bound_context(dev, ctx)
    args = (ptr(t), t.stride(0) if L > 1 else 0, t.stride(1), L, ny, nx, recs)
    check(lib.imcom_i24_compress(ctx.handle, *args, RECOGNIZED_SCHEMES.index(scheme), ptr(out), sz[3], ptr(state), state.numel() * 4, counts))
    total = sum(counts)
    oy = torch.empty(total, dtype=torch.int32, device=dev)
    ox = torch.empty(total, dtype=torch.int32, device=dev)
    ov = torch.empty(total, dtype=torch.float32, device=dev)
    if total:
        check(lib.imcom_i24_overflow_fetch(ctx.handle, *args, ptr(state), state.numel() * 4, counts, ptr(oy), ptr(ox), ptr(ov), total))
    cubes, overflows, o = [], [], 0
    for l in range(L):
        cubes.append(out[l] if scheme == "I24A" else out[l, : (recs[l].bitkeep + 7) // 8])
        overflows.append(OverflowTable(oy[o:o + counts[l]], ox[o:o + counts[l]], ov[o:o + counts[l]]))
        o += counts[l]
    return cubes, overflows


def _column(d, name, dev, index):
    """One column of an overflow table on the device; a position that no int32 holds becomes one that the kernel refuses."""
    import torch

    v = d[name]
    if is_torch(v):
        return (v.clamp(-1, 2**31 - 1).to(torch.int32) if index else v.to(torch.float32)).to(dev).contiguous()
    a = np.asarray(v)
    a = np.clip(a.astype(np.int64), -1, 2**31 - 1).astype(np.int32) if index else a.astype(np.float32)
    return staged(a, dev)


def decompress_layers(cubes, pars_list, overflows=None, ctx=None, device=None):
    """``i24decompress`` of L layers: cubes are uint8 [nb, ny, nx] (I24B) or int32 [ny, nx] (I24A), device tensors or numpy arrays (or
    one stacked array); overflows: per layer ``None`` or any object whose ``.data["y" | "x" | "value"]`` are arrays (``OverflowTable``, an
    astropy ``BinTableHDU``).  Returns float32 [L, ny, nx] on the device."""
    import torch

    dev = torch.device(device or DEVICE)
    pars_list = list(pars_list)
    recs = _records(pars_list)
    L = len(pars_list)
    whole = cubes if is_torch(cubes) and cubes.is_cuda and cubes.is_contiguous() else None  # one stacked tensor: read in place
    cubes = list(cubes)
    if len(cubes) != L or L == 0:
        raise ValueError(f"decompress_layers: {len(cubes)} cubes and {L} parameter dicts")
    kinds = [(np_dtype(c).name, len(c.shape)) for c in cubes]
    if all(k == ("uint8", 3) for k in kinds):
        scheme = "I24B"
    elif all(k == ("int32", 2) for k in kinds):
        scheme = "I24A"
    else:
        raise TypeError("decompress_layers: uint8 [nb, ny, nx] cubes (I24B) or int32 [ny, nx] images (I24A)")
    ny, nx = (int(v) for v in cubes[0].shape[-2:])
    if any(tuple(c.shape[-2:]) != (ny, nx) for c in cubes):
        raise ValueError("decompress_layers: the layers of a batch have one shape")
    _sizes(recs, ny, nx, scheme)
    for l, c in enumerate(cubes):
        if scheme == "I24B" and c.shape[0] != (recs[l].bitkeep + 7) // 8:
            raise ImcomError(-1, f"i24_decompress: a cube of {c.shape[0]} byte planes for layer {l}, BITKEEP = {recs[l].bitkeep} needs {(recs[l].bitkeep + 7) // 8}")
    ts = [staged(c, dev, layout="any") for c in cubes]
    overflows = list(overflows) if overflows is not None else [None] * L
    if len(overflows) != L:
        raise ValueError(f"decompress_layers: {len(overflows)} overflow tables and {L} layers")
    out = torch.empty((L, ny, nx), dtype=torch.float32, device=dev)
    planes = [c.shape[0] if scheme == "I24B" else 0 for c in ts]
    for g in sorted(set(planes)):  # one call for the layers of one cube depth (in practice: one)
        idx = [l for l in range(L) if planes[l] == g]
        if whole is not None and len(idx) == L:
            src = whole.to(dev)
        else:
            src = torch.stack([ts[l] for l in idx]) if len(idx) > 1 else ts[idx[0]].contiguous()[None]
        grecs = (I24Pars * len(idx))(*[recs[l] for l in idx])
        counts = (C.c_long * len(idx))()
        cols = {"y": [], "x": [], "value": []}
        for k, l in enumerate(idx):
            if overflows[l] is None:
                continue
            d = overflows[l].data
            for name in cols:
                cols[name].append(_column(d, name, dev, name != "value"))
            counts[k] = cols["y"][-1].numel()
            if cols["x"][-1].numel() != counts[k] or cols["value"][-1].numel() != counts[k]:
                raise ValueError(f"decompress_layers: the overflow columns of layer {l} differ in length")
        tab = {name: (torch.cat([c.reshape(-1) for c in v]) if v else None) for name, v in cols.items()}
        dst = out if len(idx) == L else torch.empty((len(idx), ny, nx), dtype=torch.float32, device=dev)
        ctx = bound_context(dev, ctx)
        check(lib.imcom_i24_decompress(ctx.handle, ptr(src), src[0].numel() * src.element_size(), int(g), RECOGNIZED_SCHEMES.index(scheme), len(idx), ny, nx, grecs,
                                       ptr(tab["y"]), ptr(tab["x"]), ptr(tab["value"]), counts if tab["y"] is not None else None, ptr(dst)))
        if dst is not out:
            out[idx] = dst
    return out


def i24compress(im, scheme, pars, ctx=None):
    """``pyimcom.compress.i24.i24compress`` (443-478): (data, overflow) of a 2-D float32 image.  numpy in gives numpy out; a device tensor
    in gives device tensors out and nothing crosses to the host; a torch tensor on the host comes back as torch tensors on the host.  An
    unrecognised scheme hands the input back (469-470)."""
    if scheme not in RECOGNIZED_SCHEMES:
        return im, None
    tin = is_torch(im)
    if not (len(im.shape) == 2 and (str(im.dtype) in ("float32", "torch.float32"))):
        raise TypeError("Can't initialize I24Cube: a 2D float32 image is what the device codec compresses.")
    cubes, ovs = compress_layers(im[None], [pars], scheme, ctx=ctx, device=im.device if tin and im.is_cuda else None)
    if tin and im.is_cuda:
        return cubes[0], ovs[0]
    if tin:
        return cubes[0].cpu(), OverflowTable(*(ovs[0].data[k].cpu() for k in ("y", "x", "value")))
    return cubes[0].cpu().numpy(), OverflowTable(*ovs[0].columns())


def i24decompress(im, scheme, pars, overflow=None, ctx=None):
    """``pyimcom.compress.i24.i24decompress`` (481-514): the float32 image of an I24A int32 image or an I24B uint8 cube.  numpy in gives
    numpy out, a torch tensor in a torch tensor on the device it came from.  An unrecognised scheme hands the input back (507-508)."""
    if scheme not in RECOGNIZED_SCHEMES:
        return im
    tin = is_torch(im)
    name = np_dtype(im).name
    if not ((len(im.shape) == 3 and name == "uint8") or (len(im.shape) == 2 and name == "int32")):
        raise TypeError("Can't initialize I24Cube: a 3D uint8 cube or a 2D int32 image is what the device codec decompresses.")
    out = decompress_layers([im], [pars], [overflow], ctx=ctx, device=im.device if tin and im.is_cuda else None)[0]
    if tin:
        return out if im.is_cuda else out.cpu()
    return out.cpu().numpy()
