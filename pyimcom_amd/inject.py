"""Injected star-grid layers on the device: ``GridInject.make_image_from_grid`` (reference src/pyimcom/layer.py:792-854), the image of the
``cstar`` layer and the brightness of ``nstar`` (layer.py:1346-1388), and the ``nstar`` layer made of that brightness with numpy's Poisson
draws on the device (``nstar_layer``, layer.py:1364-1387; INTEGRATION.md, seam 22).

The reference loops over the HEALPix grid points near an SCA in Python: per star one PSF out of ``InImage.get_psf_pos`` (for the cube
formats a Legendre contraction and two FFTs, coadd.py:624-640) and one ``iD5512C`` call over a 128 x 128 box.  Here the PSFs of a chunk of
stars come out of one ``imcom_psf_from_cube`` call and are drawn by one ``imcom_draw_stars`` launch (csrc/inject.hip); stars whose box
misses the chip are dropped before any PSF is formed.  ``pyimcom.layer.GridInject.make_image_from_grid =
staticmethod(pyimcom_amd.inject.make_image_from_grid)`` is the whole binding (seam 5).

Arrays may be numpy (host in, host out) or torch CUDA tensors (device in, device out, on torch's current stream)."""

import re

import numpy as np

from ._dev import bound_context, is_torch
from ._lib import MEM_DEVICE, MEM_HOST, check, default_context, lib, ptr

__all__ = ["lpoly_arr", "psf_from_cube", "draw_stars", "on_chip", "star_image", "make_image_from_grid", "make_image_from_grid_device", "parse_nstar", "nstar_layer"]

NB = 128  # tile of the library's GEMM (csrc/common.h): smooth_and_pad works on images padded to it
FILL = 0.8  # share of the free device memory a chunk is planned into


def lpoly_arr(porder, u, v):
    """``InImage.LPolyArr`` (coadd.py:476-510) for arrays of positions u, v in -1 .. +1: [S, (porder + 1)^2], the products
    P_m(u) P_n(v) with m (the x order) running fastest.  Host numpy."""
    porder = int(porder)
    u, v = np.atleast_1d(np.asarray(u, dtype=np.float64)), np.atleast_1d(np.asarray(v, dtype=np.float64))
    if porder < 0 or u.shape != v.shape or u.ndim != 1:
        raise ValueError("lpoly_arr: porder >= 0 and u, v of one length")

    def legendre(x):  # Bonnet's recurrence
        P = np.ones((x.size, porder + 1))
        if porder >= 1:
            P[:, 1] = x
        for m in range(2, porder + 1):
            P[:, m] = ((2 * m - 1) * x * P[:, m - 1] - (m - 1) * P[:, m - 2]) / m
        return P

    return np.ascontiguousarray((legendre(v)[:, :, None] * legendre(u)[:, None, :]).reshape(u.size, -1))


def pad_width(tophatwidth, gaussiansigma=0.0):
    return int(lib.imcom_smooth_pad_width(float(tophatwidth), float(gaussiansigma)))


def psf_from_cube(cube, lpoly, tophatwidth, gaussiansigma=0.0, scale=1.0, ctx=None):
    """The draw PSFs of ``InImage.get_psf_pos`` for the cube formats (coadd.py:624-640) at a batch of positions:
    ``scale * smooth_and_pad(einsum("a,aij->ij", lpoly[s], cube), tophatwidth, gaussiansigma)`` for every s.  cube [na, ny, nx], lpoly
    [S, na] -> [S, ny + 2 npad, nx + 2 npad]; scale = 1/64 for ``anlsim``, 1 for ``L2_2506``."""
    ctx = ctx or default_context()
    na, ny, nx = cube.shape
    S = int(lpoly.shape[0])
    if lpoly.ndim != 2 or lpoly.shape[1] != na:
        raise ValueError(f"lpoly shape {tuple(lpoly.shape)} does not match a cube of {na} planes")
    npad = pad_width(tophatwidth, gaussiansigma)
    shape = (S, ny + 2 * npad, nx + 2 * npad)
    if is_torch(cube):
        import torch

        cube = cube.to(torch.float64).contiguous()
        lpoly = torch.as_tensor(lpoly, dtype=torch.float64, device=cube.device).contiguous()
        out = torch.empty(shape, dtype=torch.float64, device=cube.device)
        bound_context(ctx=ctx)
        mem = MEM_DEVICE
    else:
        cube = np.ascontiguousarray(cube, dtype=np.float64)
        lpoly = np.ascontiguousarray(lpoly, dtype=np.float64)
        out = np.empty(shape)
        mem = MEM_HOST
    check(lib.imcom_psf_from_cube(ctx.handle, int(na), ptr(cube), int(ny), int(nx), S, ptr(lpoly), float(tophatwidth), float(gaussiansigma),
                                  float(scale), ptr(out), mem))
    return out


def draw_stars(psfs, xsca, ysca, nside, oversamp, d=64, out=None, ctx=None):
    """layer.py:825-852: add the stars at (xsca[s], ysca[s]) with PSF images psfs[s] (as ``psf_from_cube`` returns them, ``oversamp``
    samples per native pixel) into ``out`` [nside, nside] float64 (None: a new image of zeros) and return it.  Stars are added in
    ascending s at every pixel: the result is the same bit for bit however the list is cut into calls."""
    ctx = ctx or default_context()
    S, py, px = psfs.shape
    nside = int(nside)
    if is_torch(psfs):
        import torch

        dev = psfs.device
        psfs = psfs.to(torch.float64).contiguous()
        xsca = torch.as_tensor(xsca, dtype=torch.float64, device=dev).contiguous()
        ysca = torch.as_tensor(ysca, dtype=torch.float64, device=dev).contiguous()
        if out is None:
            out = torch.zeros((nside, nside), dtype=torch.float64, device=dev)
        elif not (is_torch(out) and out.dtype == torch.float64 and out.is_contiguous() and out.device == dev):
            raise ValueError("out must be a contiguous float64 tensor on the PSFs' device")
        bound_context(ctx=ctx)
        mem = MEM_DEVICE
    else:
        psfs = np.ascontiguousarray(psfs, dtype=np.float64)
        xsca = np.ascontiguousarray(xsca, dtype=np.float64)
        ysca = np.ascontiguousarray(ysca, dtype=np.float64)
        if out is None:
            out = np.zeros((nside, nside))
        elif not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.flags.c_contiguous):
            raise ValueError("out must be a C-contiguous float64 array")
        mem = MEM_HOST
    if tuple(out.shape) != (nside, nside) or xsca.shape[0] != S or ysca.shape[0] != S or xsca.ndim != 1 or ysca.ndim != 1:
        raise ValueError("draw_stars: out is [nside, nside], xsca and ysca have one entry per PSF")
    check(lib.imcom_draw_stars(ctx.handle, int(S), ptr(psfs), int(py), int(px), ptr(xsca), ptr(ysca), float(oversamp), int(d), nside, ptr(out), mem))
    return out


def on_chip(xsca, ysca, nside, d=64):
    """The stars the reference draws (layer.py:827-834): those whose box [int(x) - d, int(x) + d) x [int(y) - d, int(y) + d), clipped to
    the chip, keeps at least one pixel a side (int() truncates towards zero).  Positions that are not finite are off the chip."""
    keep = np.ones(np.shape(xsca), dtype=bool)
    for pos in (xsca, ysca):
        pos = np.asarray(pos, dtype=np.float64)
        fin = np.isfinite(pos) & (np.abs(pos) < 1.0e9)
        ip = np.trunc(np.where(fin, pos, 0.0)).astype(np.int64)
        keep &= fin & (np.minimum(nside, ip + d) - np.maximum(0, ip - d) >= 1)
    return keep


def _cube_workspace_bytes(na, ny, nx, npad):
    """What imcom_psf_from_cube takes from the context's workspace besides its arguments (csrc/psf_sample.hip: smooth_pad_ws_bytes,
    and the smeared planes)."""
    nyy, nxx = ny + 2 * npad, nx + 2 * npad
    Py, Px = -(-nyy // NB) * NB, -(-nxx // NB) * NB
    return 3 * na * Py * Px * 8 + Py * Py * 8 + Px * Px * 8 + (nyy + nxx) * 8 + 16384 + na * nyy * nxx * 8 + 8 * 256


def plan_chunk(nstar, psf_shape, na=0, cube_shape=None, npad=0, free_bytes=None, device=0, ctx=None):
    """Stars per chunk of ``star_image``, from exact byte counts: a chunk holds its PSFs, positions and (cube source) coefficients; the
    cube call's workspace is counted once, as far as the context does not hold it already."""
    per_star = 8 * (psf_shape[0] * psf_shape[1] + 2 + na)
    fixed = 0
    if cube_shape is not None:
        have = 0 if ctx is None or getattr(ctx, "_ws", None) is None else int(ctx._ws.numel())
        fixed = max(0, _cube_workspace_bytes(na, cube_shape[0], cube_shape[1], npad) - have)
    if free_bytes is None:
        from .stamps import free_device_bytes

        free_bytes = free_device_bytes(device)
    room = int(FILL * free_bytes) - fixed
    if room < per_star:
        raise MemoryError(f"star_image: {free_bytes} bytes free on the device, one star needs {per_star + fixed}")
    return int(max(1, min(nstar, room // per_star)))


def star_image(xsca, ysca, nside, oversamp, cube=None, lpoly=None, psf=None, psf_fn=None, chunk=None, tophatwidth=None, gaussiansigma=0.0,
               scale=1.0, d=64, out=None, device="cuda:0", ctx=None):
    """``make_image_from_grid`` after ``generate_star_grid``: the image [nside, nside] (float64 torch tensor on ``device``) of unit-flux
    stars at (xsca, ysca).  Stars whose box misses the chip are dropped before any PSF is formed (layer.py:833-834); the rest are worked
    through in ascending chunks of ``chunk`` stars (None: sized from the free device memory, ``plan_chunk``).  One PSF source:

    * ``cube`` [na, ny, nx] and ``lpoly`` [S, na] (``lpoly_arr``), with ``tophatwidth`` (None: ``oversamp``), ``gaussiansigma``, ``scale``:
      the PSFs are formed on the device (``psf_from_cube``);
    * ``psf`` [py, px]: one image for all stars (the ``dc2_imsim`` format), as ``get_psf_pos`` returns it;
    * ``psf_fn(i)`` -> [py, px] for star i of the list given: PSFs formed on the host (``piff``), uploaded per chunk."""
    import torch

    if (cube is not None) + (psf is not None) + (psf_fn is not None) != 1:
        raise ValueError("star_image: exactly one of cube, psf, psf_fn")
    ctx = ctx or default_context(torch.device(device).index or 0)
    dev = torch.device(device)
    xsca, ysca = np.asarray(xsca, dtype=np.float64).ravel(), np.asarray(ysca, dtype=np.float64).ravel()
    nside = int(nside)
    image = torch.zeros((nside, nside), dtype=torch.float64, device=dev) if out is None else out
    idx = np.nonzero(on_chip(xsca, ysca, nside, d))[0]
    if idx.size == 0:
        return image
    first = None
    if cube is not None:
        if lpoly is None or len(lpoly) != xsca.size:
            raise ValueError("star_image: lpoly has one row per star")
        tophatwidth = float(oversamp) if tophatwidth is None else float(tophatwidth)
        cube_d = torch.as_tensor(cube, dtype=torch.float64, device=dev).contiguous()
        na, ny, nx = cube_d.shape
        npad = pad_width(tophatwidth, gaussiansigma)
        shape = (ny + 2 * npad, nx + 2 * npad)
        lpoly = np.ascontiguousarray(lpoly, dtype=np.float64)
    elif psf is not None:
        psf_d = torch.as_tensor(psf, dtype=torch.float64, device=dev).contiguous()
        shape = tuple(psf_d.shape)
    else:
        first = np.asarray(psf_fn(int(idx[0])), dtype=np.float64)
        shape = first.shape
    if chunk is None:
        chunk = plan_chunk(idx.size, shape, na if cube is not None else 0, (ny, nx) if cube is not None else None,
                           npad if cube is not None else 0, device=dev, ctx=ctx)
    chunk = max(1, int(chunk))
    for c0 in range(0, idx.size, chunk):
        sel = idx[c0:c0 + chunk]
        if cube is not None:
            psfs = psf_from_cube(cube_d, torch.as_tensor(lpoly[sel], device=dev), tophatwidth, gaussiansigma, scale, ctx)
        elif psf is not None:
            psfs = psf_d.expand(sel.size, *shape)
        else:
            host = np.empty((sel.size,) + shape)
            for k, i in enumerate(sel):
                host[k] = first if (first is not None and i == idx[0]) else psf_fn(int(i))
            psfs = torch.as_tensor(host, device=dev)
        draw_stars(psfs, torch.as_tensor(xsca[sel], device=dev), torch.as_tensor(ysca[sel], device=dev), nside, oversamp, d, image, ctx)
    return image


def make_image_from_grid(res, inpsf, idsca, obsdata, mywcs, nside_sca, inpsf_oversamp, star_grid=None):
    """``GridInject.make_image_from_grid`` (layer.py:792-854) with the reference's signature: the SCA image [nside_sca, nside_sca]
    (float64, host) of the unit-flux star grid at HEALPix resolution ``res``.  ``star_grid(res, mywcs)`` -> (ipix, xsca, ysca, ra, dec)
    defaults to the reference's ``GridInject.generate_star_grid`` (HEALPix and the WCS on the host; it needs healpy) --
    ``star_grid=pyimcom_amd.healpix.generate_star_grid`` forms the grid and its positions on the device.  ``inpsf`` is
    ``InImage.get_psf_pos``: when its ``InImage`` holds a Legendre cube (``anlsim`` / ``L2_2506``) the PSFs are formed on the device
    from the cube, a ``dc2_imsim`` PSF is used for all stars, and anything else is called once per star that reaches the chip."""
    return make_image_from_grid_device(res, inpsf, idsca, obsdata, mywcs, nside_sca, inpsf_oversamp, star_grid=star_grid).cpu().numpy()


def make_image_from_grid_device(res, inpsf, idsca, obsdata, mywcs, nside_sca, inpsf_oversamp, star_grid=None):
    """``make_image_from_grid`` with its image left where it is made: the float64 tensor of ``star_image`` on the device
    (``layers.build_cube`` rounds it into the ``cstar`` plane and draws the ``nstar`` plane from it there)."""
    if star_grid is None:
        from pyimcom.layer import GridInject  # the reference package (seam 5)

        star_grid = GridInject.generate_star_grid
    ipix, xsca, ysca, rapix, decpix = star_grid(res, mywcs)
    xsca, ysca = np.asarray(xsca, dtype=np.float64), np.asarray(ysca, dtype=np.float64)
    nside = int(nside_sca)
    idx = np.nonzero(on_chip(xsca, ysca, nside))[0]
    if idx.size == 0:
        import torch

        return torch.zeros((nside, nside), dtype=torch.float64, device="cuda:0")

    def psf_fn(i):
        return inpsf((rapix[i], decpix[i]), use_drawpsf=True)

    inimage = getattr(inpsf, "__self__", None)
    cfg = getattr(getattr(inimage, "blk", None), "cfg", None)
    kw = {"psf_fn": psf_fn}
    if cfg is not None:
        draw = getattr(cfg, "inpsfdraw_format", None) is not None
        fmt = cfg.inpsfdraw_format if draw else cfg.inpsf_format
        first = psf_fn(int(idx[0]))  # get_psf_pos reads the PSF file on its first call (coadd.py:598-622)
        if fmt in ("anlsim", "L2_2506") and hasattr(inimage, "inpsf_cube") and not getattr(cfg, "psfsplit", False):
            cube = np.asarray(inimage.inpsf_cube, dtype=np.float64)
            porder = int(np.round(np.sqrt(cube.shape[0]))) - 1  # coadd.py:625-626
            wcs = getattr(inimage, "inwcs", None)
            px, py = wcs.all_world2pix(np.asarray(rapix), np.asarray(decpix), 0) if wcs is not None else (xsca, ysca)
            kw = {"cube": cube, "lpoly": lpoly_arr(porder, (np.asarray(px) - 2043.5) / 2044.0, (np.asarray(py) - 2043.5) / 2044.0),
                  "tophatwidth": float(cfg.inpsf_oversamp), "scale": 1.0 / 64.0 if fmt == "anlsim" else 1.0}
        elif fmt == "dc2_imsim":
            kw = {"psf": first}
    return star_image(xsca, ysca, nside, inpsf_oversamp, **kw)


def parse_nstar(extrainput_string):
    """``res, tot_int, bg, q`` of an ``nstar<res>,<tot_int>,<bg>,<q>`` layer name as layer.py:1357-1363 reads them; None when the string
    is no nstar layer."""
    m = re.search(r"^nstar(\d+),", extrainput_string, re.IGNORECASE)
    if not m:
        return None
    extargs = extrainput_string.split(",")[1:]
    return int(m.group(1)), float(extargs[0]), float(extargs[1]), int(extargs[2])


def nstar_layer(brightness, tot_int, bg, q, idsca, device_out=False):
    """layer.py:1364-1387 after the brightness image: the float32 ``nstar`` layer ``rng.poisson(lam=_lam) - _lam + lam - bg`` with ``lam =
    brightness * tot_int + bg``, ``_lam = np.clip(lam, 0, None)`` and ``rng = default_rng(1000000 * (18 * q + idsca[1]) + idsca[0])``, bit
    for bit.  ``brightness``: the float64 image of ``star_image`` / ``make_image_from_grid``, a tensor on the device (it stays there; no
    int64 frame is stored) or numpy.  Returns a numpy array, or with ``device_out`` the tensor on the device.  A request the device
    cannot decide (``noiselayers.last_poisson_info["undecided"]``) is drawn by numpy on the host."""
    from . import noiselayers as nl

    tot_int, bg = float(tot_int), float(bg)
    seed = 1000000 * (18 * int(q) + int(idsca[1])) + int(idsca[0])
    if not is_torch(brightness):
        brightness = np.ascontiguousarray(brightness, dtype=np.float64)
    shape = tuple(int(s) for s in brightness.shape)
    device = brightness.device if is_torch(brightness) and brightness.is_cuda else ("cuda:0" if device_out else None)

    def call(ctx, stream, values, count, out, info, mem):
        return lib.imcom_nstar_layer(ctx.handle, *stream, values, tot_int, bg, count, out, info, mem)

    def host(gen, b):
        lam = b.reshape(shape) * tot_int + bg
        _lam = np.clip(lam, 0, None)
        return (gen.poisson(lam=_lam) - _lam + lam - bg).astype(np.float32)

    out, _ = nl._poisson_call(np.random.PCG64(seed), 0, brightness, shape, np.float32, device, call, host, "nstar_layer")
    if is_torch(out):
        return out if device_out else out.cpu().numpy()
    if device_out:
        import torch

        return torch.from_numpy(out).to("cuda:0")
    return out
