"""Noise power spectra of coadded blocks on the device: the numerical content of ``pyimcom.analysis.NoiseAnal.__call__`` (reference
src/pyimcom/analysis.py:745-807), of the loop of ``_BlkGrp.get_noise_power_spectra`` (1202-1307) and of
``diagnostics.noise_diagnostics.NoiseReport.measure_power_spectrum`` / ``azimuthal_average`` (noise_diagnostics.py:400-506).

The device does the passes over the frames (csrc/noisespec.hip): the real 2-D transform in float64, |F|^2 / norm folded to the shifted full
spectrum, the 8 x 8 averages, the azimuthal average with its standard error, and the sums over the blocks of a mosaic.  The host keeps what
is small or is not arithmetic: the label image, the wavenumbers, the coverage bins, the Tukey window (the reference builds it with
``skimage.filters.window``; the caller builds it once per mosaic and hands it over) and the files.

A numpy input gives numpy results; a torch tensor on the device gives torch results with no host round trip.  INTEGRATION.md, seam 9."""

import numpy as np

from ._dev import bound_context, is_torch, staged, to_host
from ._lib import MEM_DEVICE, check, lib, ptr

__all__ = ["power_spectrum_2d", "windowed_norm", "radial_labels", "azimuthal_average", "wavenumbers", "NoiseSpectra", "noise_anal_call", "get_norm",
           "route", "ROUTE_LINES", "ROUTE_DENSE", "ROUTE_TWOLEVEL"]

FILL = 0.8  # share of the free device memory a chunk plan may use
ROUTE_LINES, ROUTE_DENSE, ROUTE_TWOLEVEL = 1, 2, 3  # csrc/noisespec.hip: wave-per-line butterflies, dense DFT on the MFMA engine, N1 x N2 lines in LDS
MAXN = 4096


def route(L):
    """How a side is served: ROUTE_LINES, ROUTE_TWOLEVEL, ROUTE_DENSE, or 0 (odd, or beyond 4096).  ``IMCOM_NOISEPS_ROUTE=dense`` in the
    environment forces the dense route."""
    return int(lib.imcom_noiseps_route(int(L)))


def _sizes(L, nframe, bin8, route_=0):
    out = np.zeros(4, dtype=np.int64)
    check(lib.imcom_noiseps_sizes(int(L), int(nframe), int(bool(bin8)), int(route_), ptr(out)))
    return out


def _check_side(L, bin8):
    if L < 2 or L % 2 != 0:
        raise ValueError(f"noise spectra: the side {L} is not even")
    if bin8 and L % 8 != 0:
        raise ValueError(f"noise spectra: the side {L} is not a multiple of 8 (8 x 8 binning)")
    if L > MAXN:
        raise ValueError(f"noise spectra: a side of {L} is beyond the {MAXN} this build transforms")


def _plan_frames(L, nframe, bin8, route_, free_bytes):
    """Frames per call from exact byte counts."""
    room = int(FILL * free_bytes)
    k = nframe
    while k > 1 and int(_sizes(L, k, bin8, route_)[2]) > room:
        k = (k + 1) // 2
    need = int(_sizes(L, k, bin8, route_)[2])
    if need > room:
        raise MemoryError(f"noise spectra: {free_bytes} bytes free on the device, one frame of side {L} needs {need}")
    return k


def windowed_norm(norm, w):
    """noise_diagnostics.py:432: the norm of a windowed frame, ``norm * mean(w^2)``."""
    w = to_host(w)
    return norm * np.average(w.astype(np.float64) ** 2)


def power_spectrum_2d(frames, norm=1.0, window=None, bin8=True, ctx=None, route=0, frames_per_call=None, device="cuda:0"):
    """``ps[ky, kx] = |fftshift(fft2(frame * window))|^2 / norm`` (analysis.py:789-793, noise_diagnostics.py:430-436), with ``bin8`` averaged
    over 8 x 8 cells (794 / 439).  ``frames``: [L, L] or [n, L, L], float32 or float64, numpy or a torch tensor on the device (views are read
    in place when their last stride is 1); ``norm``: a number or one per frame (with a window the caller passes ``windowed_norm(norm, w)``);
    ``window``: float64 [L, L] or None.  Returns float64 [L/8, L/8] or [L, L] per frame, of the kind of the input.  The result of a frame
    does not depend on the other frames of the call or on ``frames_per_call``, bit for bit."""
    import torch

    from .stamps import free_device_bytes

    torch_in = is_torch(frames)
    shape = tuple(frames.shape)
    if len(shape) not in (2, 3) or shape[-1] != shape[-2]:
        raise ValueError("frames is [L, L] or [n, L, L]")
    L, single = int(shape[-1]), len(shape) == 2
    _check_side(L, bin8)
    if window is not None and tuple(window.shape) != (L, L):
        raise ValueError(f"a window of shape {tuple(window.shape)} for frames of side {L}")
    if torch_in:
        if not (frames.is_cuda and frames.dtype in (torch.float32, torch.float64)):
            raise ValueError("torch frames must be a float32 or float64 tensor on the device")
        dev = frames.device
        t = frames[None] if single else frames
        if t.stride(2) != 1 or t.stride(1) < L or (t.shape[0] > 1 and t.stride(0) < (L - 1) * t.stride(1) + L):
            t = t.contiguous()
    else:
        dev = torch.device(device)
        a = np.asarray(frames)
        t = staged(a[None] if single else a, dev, astype=None if a.dtype in (np.float32, np.float64) else np.float64)
    nframe = int(t.shape[0])
    if nframe < 1:
        raise ValueError("no frames")
    norms = np.ascontiguousarray(np.broadcast_to(np.asarray(norm, dtype=np.float64), (nframe,)))
    w = None
    if window is not None:
        w = staged(window, dev, astype=np.float64)
    ctx = bound_context(dev, ctx)
    n = L // 8 if bin8 else L
    out = torch.empty((nframe, n, n), dtype=torch.float64, device=dev)
    step = int(frames_per_call) if frames_per_call else _plan_frames(L, nframe, bin8, route, free_device_bytes(dev))
    fstride = int(t.stride(0)) if nframe > 1 else L * int(t.stride(1))
    for f0 in range(0, nframe, step):
        k = min(step, nframe - f0)
        check(lib.imcom_noiseps_2d(ctx.handle, ptr(t[f0]), int(t.dtype == torch.float64), k, L, fstride, int(t.stride(1)), ptr(w), 0 if w is None else L * L,
                                   ptr(norms[f0:f0 + k]), int(bool(bin8)), int(route), ptr(out[f0]), MEM_DEVICE))
    torch.cuda.current_stream(dev).synchronize()  # uploaded copies go back to the allocator
    res = out[0] if single else out
    return res if torch_in else res.cpu().numpy()


def radial_labels(n, nradbins):
    """analysis.py:691-695 (and 1260-1262): the annulus label of every pixel of an [n, n] image, ``int(nradbins r / r_max)`` with r the distance
    from (n / 2, n / 2).  The one pixel with the largest label is the corner (0, 0)."""
    yy, xx = np.mgrid[:n, :n]
    r = np.hypot(xx - n / 2, yy - n / 2)
    return (nradbins * r / r.max()).astype(int)


def azimuthal_average(image, nradbins, rbin=None, ridx=None, ctx=None, device="cuda:0"):
    """``NoiseAnal.azimuthal_average`` (analysis.py:661-704; noise_diagnostics.py:472-506 without its ``r``): ``(mean, err)`` over the annuli
    1 .. rbin.max() of ``image`` [n, n] or [f, n, n] (float64), ``err = std / sqrt(npix)`` with the two-pass standard deviation of
    ``ndimage.standard_deviation``.  ``rbin`` may be a numpy array or an int32 tensor on the device; a ``ridx`` other than
    ``arange(1, rbin.max() + 1)`` is refused."""
    import torch

    torch_in = is_torch(image)
    shape = tuple(image.shape)
    if len(shape) not in (2, 3) or shape[-1] != shape[-2]:
        raise ValueError("image is [n, n] or [f, n, n]")
    n, single = int(shape[-1]), len(shape) == 2
    if rbin is None:
        rbin = radial_labels(n, nradbins)
    if tuple(rbin.shape) != (n, n):
        raise ValueError(f"labels of shape {tuple(rbin.shape)} for an image of side {n}")
    nidx = int(rbin.max())
    if ridx is not None:
        r = to_host(ridx)
        if r.shape != (nidx,) or not np.array_equal(r, np.arange(1, nidx + 1)):
            raise ValueError("ridx must be arange(1, rbin.max() + 1)")
    if nidx < 1:
        raise ValueError("the labels hold no annulus")
    if torch_in:
        if not (image.is_cuda and image.dtype == torch.float64):
            raise ValueError("a torch image must be a float64 tensor on the device")
        dev = image.device
        img = image.contiguous()
    else:
        dev = torch.device(device)
        img = staged(image, dev, astype=np.float64)
    lab = staged(rbin, dev, astype=np.int32)
    nframe = 1 if single else int(shape[0])
    ctx = bound_context(dev, ctx)
    mean = torch.empty((nframe, nidx), dtype=torch.float64, device=dev)
    err = torch.empty_like(mean)
    check(lib.imcom_noiseps_radial(ctx.handle, ptr(img), nframe, n, ptr(lab), nidx, ptr(mean), ptr(err), MEM_DEVICE))
    torch.cuda.current_stream(dev).synchronize()
    if single:
        mean, err = mean[0], err[0]
    return (mean, err) if torch_in else (mean.cpu().numpy(), err.cpu().numpy())


def wavenumbers(L, nradbins):
    """``NoiseAnal._get_wavenumbers(L, nradbins)`` (analysis.py:707-743): the mean |k| (cycles per pixel) of the annuli of an [L, L] grid.
    On the host: once per mosaic."""
    k = np.fft.fftshift(np.fft.fftfreq(L))
    kx, ky = np.meshgrid(k, k)
    k = np.sqrt(np.square(kx) + np.square(ky))
    rbin = radial_labels(L, nradbins).ravel()
    nidx = int(rbin.max())
    return np.bincount(rbin, weights=k.ravel(), minlength=nidx + 1)[1:] / np.bincount(rbin, minlength=nidx + 1)[1:]


def get_norm(layer, L, s_out, *, lab_norm=None):
    """``NoiseAnal.get_norm`` (analysis.py:645-658) for the simulated layers: ``(L / s_out)^2`` for "white..." and "1f..."; a "lab..." layer
    takes the caller's ``lab_norm`` (its unit conversion is the host's)."""
    if layer.startswith(("white", "1f")):
        return (L / s_out) ** 2
    if layer.startswith("lab") and lab_norm is not None:
        return lab_norm
    raise ValueError(f"no norm for the layer {layer!r}")


class NoiseSpectra:
    """The accumulators of ``_BlkGrp.get_noise_power_spectra`` (analysis.py:1253-1303) on the device.  ``L``: the side of the frames (a
    multiple of 8 with ``bin8``), ``nlayers`` noise layers, ``bins`` coverage bins.  ``add(frames, coverage_bin)`` takes the ``nlayers``
    frames of one block ([nlayers, L, L], a view of the block on the device or numpy) in the loop's order; ``result`` applies the divisions."""

    def __init__(self, L, nlayers, bins, bin8=True, window=None, norm=1.0, ctx=None, device="cuda:0"):
        import torch

        _check_side(L, bin8)
        self.L, self.nlayers, self.bins, self.bin8 = int(L), int(nlayers), int(bins), bool(bin8)
        self.dev = torch.device(device)
        self.ctx = bound_context(self.dev, ctx)
        self.n = self.L // 8 if bin8 else self.L
        self.nradbins = self.L // 16  # 1257-1259
        self.rbin = radial_labels(self.n, self.nradbins)  # 1260-1262
        self.ridx = np.arange(1, self.rbin.max() + 1)
        self._rbin_dev = staged(self.rbin, self.dev, astype=np.int32)
        self.window = None if window is None else torch.as_tensor(np.asarray(window, dtype=np.float64), device=self.dev)
        self.norm = np.broadcast_to(np.asarray(norm if window is None else windowed_norm(norm, window), dtype=np.float64), (self.nlayers,)).copy()
        self.wavenumbers = wavenumbers(self.L, self.nradbins)  # 1266 (the caller divides by s_out, 1268)
        f64 = dict(dtype=torch.float64, device=self.dev)
        self.ps2d_all = torch.zeros((self.nlayers, self.n, self.n), **f64)
        self.ps1d_all = torch.zeros((self.nlayers, self.bins, len(self.ridx), 2), **f64)
        self.nadded = 0

    def add(self, frames, coverage_bin):
        """1276-1279 for the layers of one block."""
        import torch

        if tuple(frames.shape) != (self.nlayers, self.L, self.L):
            raise ValueError(f"frames of shape {tuple(frames.shape)}, not {(self.nlayers, self.L, self.L)}")
        if not 0 <= int(coverage_bin) < self.bins:
            raise ValueError(f"coverage bin {coverage_bin} of {self.bins}")
        if not is_torch(frames):
            a = np.asarray(frames)
            frames = staged(a, self.dev, astype=None if a.dtype in (np.float32, np.float64) else np.float64)
        ps2d = power_spectrum_2d(frames, self.norm, self.window, self.bin8, ctx=self.ctx)
        mean, err = azimuthal_average(ps2d, self.nradbins, self._rbin_dev, ctx=self.ctx)
        bound_context(ctx=self.ctx)
        check(lib.imcom_noiseps_accumulate(self.ctx.handle, ptr(ps2d), ptr(mean), ptr(err), self.nlayers, self.n, len(self.ridx), self.bins, int(coverage_bin),
                                           ptr(self.ps2d_all), ptr(self.ps1d_all)))
        torch.cuda.current_stream(self.dev).synchronize()  # ps2d, mean, err go back to the allocator
        self.nadded += 1

    def result(self, count_per_bin, nblocks):
        """1297-1303: ``ps2d_all / nblocks`` and ``ps1d_all[:, bin] / count`` for the bins with a count, as numpy arrays in the layout of the
        reference's ``_NoisePS.npz``: (ps2d_all, ps1d_all, wavenumbers)."""
        ps2d = self.ps2d_all.cpu().numpy() / nblocks
        ps1d = self.ps1d_all.cpu().numpy()
        for idx, count in enumerate(count_per_bin):
            if count:
                ps1d[:, idx, :, :] /= count
        return ps2d, ps1d, self.wavenumbers.copy()


def noise_anal_call(self, padding=False, bin_=True, rbin=None, ridx=None):
    """``NoiseAnal.__call__`` (analysis.py:745-807) with its signature and effects (``self.ps2d`` float64 [Lcut/8, Lcut/8], ``self.ps1d``
    [Lcut/16, 2]); bind as ``pyimcom.analysis.NoiseAnal.__call__ = pyimcom_amd.noisespec.noise_anal_call``.  As in the reference ``bin_`` is
    ignored.  The norm is ``NoiseAnal.get_norm`` of the object's own class when it has one (the lab layers' unit conversion stays there)."""
    L = self.cfg.NsideP
    indata = self.outim.get_coadded_layer(self.layer)
    if not padding:
        L = self.cfg.Nside
        bdpad = self.cfg.n2 * self.cfg.postage_pad
        indata = indata[bdpad:-bdpad, bdpad:-bdpad]
    s_out = self.cfg.dtheta * 3600.0  # degrees to arcsec (784)
    Lcut = L // 8 * 8
    getn = getattr(type(self), "get_norm", None)
    if getn is not None:
        filt = getattr(self, "filtername", None)
        if filt is None:
            from importlib import import_module

            try:
                filt = import_module("pyimcom.config").Settings.RomanFilters[self.cfg.use_filter]
            except ImportError:
                filt = self.cfg.use_filter
        norm = getn(self.layer, Lcut, filt, s_out)
    else:
        norm = get_norm(self.layer, Lcut, s_out)
    self.ps2d = power_spectrum_2d(indata[:Lcut, :Lcut], norm, None, True)
    nradbins = Lcut // 16
    mean, err = azimuthal_average(self.ps2d, nradbins, rbin, ridx)
    if is_torch(mean):
        import torch

        self.ps1d = torch.stack((mean, err), dim=1)
    else:
        self.ps1d = np.zeros((Lcut // 16, 2))
        self.ps1d[:, 0] = mean
        self.ps1d[:, 1] = err
