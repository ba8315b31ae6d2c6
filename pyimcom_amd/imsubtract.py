"""The long-range PSF part of an SCA image, subtracted on the device: the convolution at the heart of
``pyimcom.splitpsf.imsubtract.run_imsubtract_single`` (reference src/pyimcom/splitpsf/imsubtract.py:689-707, with ``fftconvolve_multi``,
imsubtract.py:48-142) and the canvas assembly that feeds it (imsubtract.py:658-682).

The reference convolves the ``A x A`` canvas (A = oversamp * (nside + 2 I_pad), about 33 000 for an SCA) ``Nl^2`` times at full resolution
and keeps one sample in ``oversamp^2``.  Here only the kept samples are formed (csrc/imsubtract.hip): the sum splits exactly into
``oversamp^2`` phases, each a dense correlation of an ``(ax / oversamp)^2`` kernel with a sub-image of the canvas; one thread owns an output
sample and adds its terms in a fixed order in float64, so a layer is the same bit for bit for every split of its rows into calls.

Arrays may be numpy (host, memory maps included: the canvas is then uploaded in the row bands the plan cuts) or torch CUDA tensors.
INTEGRATION.md, seam 6, has the lines that replace imsubtract.py:689-707."""

import math

import numpy as np

from ._dev import bound_context, device_of, is_torch, staged, to_host
from ._lib import MEM_DEVICE, MEM_HOST, check, default_context, lib, ptr

__all__ = ["geometry", "legendre_order", "phase_tables", "prepare_kernel", "plan_bands", "canvas_add", "subtract_long_range", "LongRangeSubtractor"]

FILL = 0.8  # share of the free device memory a band plan may use
TILE_ROWS = 32  # output rows of a workgroup (csrc/imsubtract.hip: IMS_TY); bands are cut at multiples of it


def geometry(axis_num, oversamp, nside):
    """imsubtract.py:365-366, 387-389, 451: (I_pad, first_index, A) for kernel planes of ``axis_num`` samples a side.  ``axis_num`` is a
    multiple of ``2 * oversamp``, or -- the kernels ``bin2x2`` trims (imsubtract.py:373-376) -- a multiple of an odd ``oversamp``."""
    ax, s, nside = int(axis_num), int(oversamp), int(nside)
    if s < 2 or ax < s or nside < 1:
        raise ValueError(f"imsubtract: oversamp={s}, axis_num={ax}, nside={nside}")
    if ax % (2 * s) and not (s % 2 == 1 and ax % s == 0):
        raise ValueError(f"axis_num={ax} must be a multiple of 2*oversamp, oversamp={s}")
    I_pad = int(math.ceil(ax / 2 / s))
    return I_pad, (s + 2 * s * I_pad - ax) // 2, s * (nside + 2 * I_pad)


def legendre_order(ncoeff, porder=-1):
    """imsubtract.py:482-485: the ``Nl`` of the double loop -- PORDER_IMSUBTRACT itself when it is not negative."""
    Nl = int(porder) if int(porder) >= 0 else int(math.floor(math.sqrt(int(ncoeff) + 0.5)))
    if Nl * Nl > int(ncoeff):
        raise ValueError(f"imsubtract: Nl={Nl} needs {Nl * Nl} kernel planes, the cube has {int(ncoeff)}")
    return Nl


def phase_tables(axis_num, oversamp, first_index):
    """For the kernel phase p (rows j = oversamp * j' + p; the same table serves the columns): the residue ``rho[p]`` modulo oversamp of the
    canvas rows that phase reads and the offset ``B[p]``: output row Y and flipped kernel row jj = ax/oversamp - 1 - j' meet at canvas row
    ``oversamp * (Y + B[p] + jj) + rho[p]``."""
    ax, s = int(axis_num), int(oversamp)
    e = int(first_index) + ax - 1 - np.arange(s)
    return e % s, e // s - (ax // s - 1)


def _reinterp(arr):
    """imsubtract.py:241-262: arr [2N+2, 2N+2] -> [N, N], the cubic midpoint interpolation at double spacing (separable, float64 here)."""
    f = np.array([-0.125, 1.125, 1.125, -0.125], dtype=np.float32).astype(np.float64)
    n = (arr.shape[0] - 2) // 2, (arr.shape[1] - 2) // 2
    a = np.asarray(arr, dtype=np.float64)
    rows = sum(f[k] * a[3 - k:3 - k + 2 * n[0]:2, :] for k in range(4))
    return sum(f[k] * rows[:, 3 - k:3 - k + 2 * n[1]:2] for k in range(4))


def prepare_kernel(K, oversamp, bin2x2=False):
    """imsubtract.py:365-384: the kernel cube as the convolution uses it -> (K float32 [ncoeff, axis_num, axis_num], oversamp).  With
    ``bin2x2`` the planes are re-interpolated at half the sampling after the reference's trim (odd halved oversamp) or edge pad."""
    K = np.asarray(K)
    s, ax = int(oversamp), K.shape[1]
    if K.ndim != 3 or K.shape[2] != ax:
        raise ValueError("prepare_kernel: K is [ncoeff, axis_num, axis_num]")
    if ax % (2 * s):
        raise ValueError(f"axis_num={ax} must be a multiple of 2*oversamp, oversamp={s}")
    if not bin2x2:
        return np.ascontiguousarray(K, dtype=np.float32), s
    if s % 2:
        raise ValueError(f"oversamp={s:d} is odd, not consistent with bin2x2")
    s //= 2
    ax //= 2
    if s % 2 and not ax // s % 2:
        K = K[:, s - 1:1 - s, s - 1:1 - s]
    else:
        K = np.pad(K, ((0, 0), (1, 1), (1, 1)), mode="edge")
    return np.ascontiguousarray(np.stack([_reinterp(k) for k in K]), dtype=np.float32), s


def band_rows(y0, ny, axis_num, oversamp, first_index):
    """The canvas rows [lo, hi) that the output rows y0 .. y0 + ny - 1 read."""
    return first_index + oversamp * y0, first_index + oversamp * (y0 + ny - 1) + axis_num


def plan_bands(nside, axis_num, oversamp, Nl, free_bytes, canvas_on_device, kernel_resident=True):
    """Cut the ``nside`` output rows into bands [(y0, ny), ...] from exact byte counts.  A band holds, besides what is resident, the canvas
    rows it reads (host canvases only: a device canvas is read in place), and the Legendre table; the image and the optional sums are the
    caller's tensors.  Bands are multiples of TILE_ROWS rows; the result does not depend on the cut."""
    I_pad, first, A = geometry(axis_num, oversamp, nside)
    ax, s = int(axis_num), int(oversamp)
    np_ = ax // s
    fixed = 4 * Nl * A + 256 + (0 if kernel_resident else 8 * Nl * Nl * s * s * np_ * (-(-np_ // 8) * 8) + 256)
    room = int(FILL * free_bytes) - fixed
    per_row = 0 if canvas_on_device else 4 * A * s
    base = 0 if canvas_on_device else 4 * A * (ax - s)
    if per_row == 0:
        rows = nside
    else:
        rows = (room - base) // per_row // TILE_ROWS * TILE_ROWS
        if rows < TILE_ROWS:
            raise MemoryError(f"imsubtract: {free_bytes} bytes free on the device, a band of {TILE_ROWS} rows needs {fixed + base + per_row * TILE_ROWS}")
    rows = int(min(rows, nside))
    return [(y0, min(rows, nside - y0)) for y0 in range(0, nside, rows)]


def canvas_add(canvas, H, area, oversamp, bottom, left, ctx=None):
    """imsubtract.py:665-682: ``canvas[bottom:bottom + h, left:left + w] += H * area`` with the native-pixel ``area`` [h / oversamp,
    w / oversamp] replicated over oversamp x oversamp samples; bottom, left in canvas samples (oversamp * (bottom + I_pad) there).  canvas
    float32 [A, A], updated in place and returned."""
    ctx = ctx or default_context()
    s = int(oversamp)
    hh, hw = H.shape
    if is_torch(canvas):
        import torch

        if not (canvas.dtype == torch.float32 and canvas.is_contiguous() and canvas.ndim == 2 and canvas.shape[0] == canvas.shape[1]):
            raise ValueError("canvas must be a contiguous square float32 tensor")
        H = torch.as_tensor(H, dtype=torch.float64, device=canvas.device).contiguous()
        area = torch.as_tensor(area, dtype=torch.float32, device=canvas.device).contiguous()
        bound_context(ctx=ctx)
        mem = MEM_DEVICE
    else:
        if not (isinstance(canvas, np.ndarray) and canvas.dtype == np.float32 and canvas.flags.c_contiguous and canvas.ndim == 2
                and canvas.shape[0] == canvas.shape[1]):
            raise ValueError("canvas must be a C-contiguous square float32 array")
        H = np.ascontiguousarray(H, dtype=np.float64)
        area = np.ascontiguousarray(area, dtype=np.float32)
        mem = MEM_HOST
    if hh % s or hw % s or tuple(area.shape) != (hh // s, hw // s):
        raise ValueError(f"canvas_add: H is {hh} x {hw}, area {tuple(area.shape)}, oversamp {s}")
    check(lib.imcom_imsub_canvas_add_f32(ctx.handle, ptr(canvas), int(canvas.shape[0]), ptr(H), hh, hw, ptr(area), s, int(bottom), int(left), mem))
    return canvas


class LongRangeSubtractor:
    """The kernel of one SCA, prepared once and kept on the device over its layers.

        sub = LongRangeSubtractor(K, oversamp, nside, porder=cfg.porder_imsubtract)   # K [Ncoeff, axis_num, axis_num], after prepare_kernel
        for n in range(nlayer):
            I_img[n] = sub.subtract(I_img[n], H_canvas)

    ``subtract`` takes the layer (float32 [nside, nside]) and the canvas (float32 [A, A]) as numpy arrays -- the canvas may be a memory map;
    it is uploaded in the row bands ``plan_bands`` cuts from the free device memory -- or as torch tensors on the device."""

    def __init__(self, K, oversamp, nside, porder=-1, device="cuda:0", ctx=None):
        import torch

        self.dev = torch.device(device)
        self.ctx = bound_context(self.dev, ctx)
        K = to_host(K)
        if K.ndim != 3 or K.shape[1] != K.shape[2]:
            raise ValueError("K is [ncoeff, axis_num, axis_num]")
        self.ncoeff, self.ax = int(K.shape[0]), int(K.shape[1])
        self.s, self.nside = int(oversamp), int(nside)
        self.Nl = legendre_order(self.ncoeff, porder)
        self.I_pad, self.first, self.A = geometry(self.ax, self.s, self.nside)
        if self.Nl < 1:
            self.kf = None  # PORDER_IMSUBTRACT = 0: the reference's loop has no term
            return
        sz = np.zeros(6, dtype=np.int64)
        check(lib.imcom_imsub_sizes(self.ax, self.s, self.nside, self.Nl, ptr(sz)))
        self.kf = torch.empty(int(sz[5]), dtype=torch.float64, device=self.dev)
        planes = staged(K[:self.Nl * self.Nl], self.dev, astype=np.float32)
        bound_context(ctx=self.ctx)
        check(lib.imcom_imsub_prepare_kernel_f32(self.ctx.handle, ptr(planes), self.Nl * self.Nl, self.ax, self.Nl, self.s, ptr(self.kf), MEM_DEVICE))
        torch.cuda.current_stream(self.dev).synchronize()  # `planes` is dropped on return

    def plan(self, canvas_on_device, free_bytes=None):
        if free_bytes is None:
            from .stamps import free_device_bytes

            free_bytes = free_device_bytes(self.dev)
        return plan_bands(self.nside, self.ax, self.s, self.Nl, free_bytes, canvas_on_device)

    def subtract(self, image, canvas, bands=None, return_kh=False):
        """image -= the decimated long-range convolution of ``canvas`` (imsubtract.py:689-707).  Returns the layer (a host array is updated
        in place), with ``return_kh`` also the float64 sums [nside, nside].  ``bands``: [(y0, ny), ...] instead of the plan's."""
        import torch

        nside, A, s, ax = self.nside, self.A, self.s, self.ax
        if tuple(image.shape) != (nside, nside):
            raise ValueError(f"image is {tuple(image.shape)}, the SCA {nside} x {nside}")
        if tuple(canvas.shape) != (A, A):
            raise ValueError(f"canvas is {tuple(canvas.shape)}, oversamp * (nside + 2 * I_pad) = {A}")
        host_image = not is_torch(image)
        if host_image:
            if not (isinstance(image, np.ndarray) and image.dtype == np.float32):
                raise ValueError("image must be a float32 array")
            img_d = staged(image, self.dev)
        else:
            if not (image.dtype == torch.float32 and image.is_contiguous() and image.device == self.dev):
                raise ValueError("image must be a contiguous float32 tensor on the subtractor's device")
            img_d = image
        kh = torch.zeros((nside, nside), dtype=torch.float64, device=self.dev) if return_kh else None
        if self.kf is not None:
            on_dev = is_torch(canvas)
            if on_dev and not (canvas.dtype == torch.float32 and canvas.is_contiguous() and canvas.device == self.dev):
                raise ValueError("canvas must be a contiguous float32 tensor on the subtractor's device")
            if not on_dev and canvas.dtype != np.float32:
                raise ValueError("canvas must be float32")
            bound_context(ctx=self.ctx)
            for y0, ny in (bands if bands is not None else self.plan(on_dev)):
                lo, hi = band_rows(y0, ny, ax, s, self.first)
                band = canvas if on_dev else torch.from_numpy(np.array(canvas[lo:hi], dtype=np.float32, order="C", subok=False)).to(self.dev)
                crow0, crows = (0, A) if on_dev else (lo, hi - lo)
                check(lib.imcom_imsub_convolve_subtract_f32(self.ctx.handle, ptr(band), A, crow0, crows, None, ptr(self.kf), self.ncoeff, ax, self.Nl, s,
                                                            nside, int(y0), int(ny), ptr(img_d[y0:y0 + ny]), None if kh is None else ptr(kh[y0:y0 + ny]),
                                                            MEM_DEVICE))
                if not on_dev:
                    torch.cuda.current_stream(self.dev).synchronize()  # the band goes back to the allocator before the next one is cut
                    del band
        if host_image:
            image[...] = img_d.cpu().numpy()
            out = image
        else:
            out = img_d
        if return_kh:
            return out, (kh.cpu().numpy() if host_image else kh)
        return out


def subtract_long_range(image, canvas, K, *, oversamp, nside, porder=-1, bands=None, return_kh=False, ctx=None):
    """One layer of imsubtract.py:689-707: ``image -= KH[first_index::oversamp, first_index::oversamp]`` for the canvas ``canvas`` and the
    kernel cube ``K`` [Ncoeff, axis_num, axis_num] (``prepare_kernel`` first for ``bin2x2``); ``porder`` is PORDER_IMSUBTRACT.  For
    several layers of one SCA keep a ``LongRangeSubtractor``."""
    dev = device_of(image, canvas)
    return LongRangeSubtractor(K, oversamp, nside, porder, device=dev, ctx=ctx).subtract(image, canvas, bands=bands, return_kh=return_kh)
