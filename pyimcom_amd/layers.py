"""The input-layer cube on the device: ``pyimcom.layer.get_all_data`` (reference src/pyimcom/layer.py:1199-1527), which fills
``inimage.indata [n_inframe, nside, nside]`` float32 for one exposure from ``cfg.extrainput`` (seam 23).

The generated layers have device seams of their own (``whitenoise`` / ``1fnoise``: ``noiselayers``; ``cstar`` / ``nstar``: ``inject``) and the
consumers take a device tensor (``simmask.load_cr_mask``, ``inpool.Partition.extract_layers`` / ``PoolBuilder.add_image``).  ``build_cube``
joins them: the reference's loop over ``extrainput`` with its quirks, every generated plane made where the cube lives, and every other
plane -- the science frame minus its sky, truth, labnoise, skyerr, a saved noise slice, a GalSim layer -- placed by one kernel
(``imcom_layer_place``, csrc/layers.hip) from the bytes as the file holds them: a big-endian FITS image is uploaded raw and swapped as it is
read, with numpy >= 2's arithmetic (layers_core.h).  Only file bytes cross to the device.  The binding is

    pyimcom.coadd.get_all_data = pyimcom_amd.layers.get_all_data          # coadd.py:45 imports the name

``FileSources`` and the two default ``inlayercache`` hooks restate the reference's file statements and need astropy, asdf, filelock and the
reference package; none of them is installed where this library is built, so they are UNVERIFIED (as ``healpy`` is for seams 5 and 18), and
the default GalSim provider likewise.  Everything else is tested through in-memory ``sources``.

One deviation: a source whose shape numpy would merely broadcast into the plane (``(1, nside)``, ``(1, 1)``, a leading axis of one) is refused
with ``ValueError``; the reference would smear it over the plane."""

import re
import warnings
from collections import OrderedDict

import numpy as np

from ._dev import DEVICE, bound_context, is_torch
from ._lib import MEM_DEVICE, ImcomError, check, lib, ptr

__all__ = ["layer_seed", "pick_noise_slice", "galsim_kind", "place", "build_cube", "get_all_data", "FileSources", "CubeCache", "SOURCE_TYPES"]

IMCOM_ERR_UNSUPPORTED = -4
SOURCE_TYPES = {"float32": 0, "float64": 1, "int16": 2, "uint16": 3, "int32": 4, "uint8": 5}  # src_type of imcom_layer_place (layers_core.h)
FLIP_NONE, FLIP_X, FLIP_Y = 0, 1, 2
FITS_FORMATS = ("dc2_imsim", "anlsim")  # layer.py:1259: the SCI frame of a FITS file, the sky in its header
ASDF_FORMATS = ("L2_2506",)  # layer.py:1262
GALSIM_TESTS = (("gsstar", r"^gsstar(\d+)$"), ("gstrstar", r"^gstrstar(\d+)$"), ("gsfdstar", r"^gsfdstar(\d+),(.+)+$"), ("gsext", r"^gsext(\d+)"),
                ("gsextchrom", r"^gsextchrom(\d+)"))  # layer.py:1391, 1401, 1419, 1436, 1446, in the reference's order


def layer_seed(q, idsca):
    """The seed of the generated layer with index ``q`` of exposure ``idsca`` = (obsid, sca): layer.py:1301, 1311, 1364."""
    return 1000000 * (18 * int(q) + int(idsca[1])) + int(idsca[0])


def pick_noise_slice(labels, label, filename=""):
    """layer.py:1467-1488: the index of the first entry of ``labels`` equal to ``label`` (with the reference's warning when a second one
    follows), or -1 with its warning when there is none."""
    jn_use = -1
    for jn in range(len(labels)):
        if labels[jn] == label:
            if jn_use >= 0:
                warnings.warn("label " + label + " repeated in " + filename + ": using first instance")
                break
            jn_use = jn
    if jn_use < 0:
        warnings.warn("WARNING: cannot find slice " + label + " in " + filename + ": continuing")
    return jn_use


def galsim_kind(name):
    """Which GalSim layer ``name`` is: the last of the reference's five tests (``GALSIM_TESTS``) that matches -- a later match overwrites an
    earlier one's plane -- or None."""
    kind = None
    for k, pattern in GALSIM_TESTS:
        if re.search(pattern, name, re.IGNORECASE):
            kind = k
    return kind


def flip_of(informat, idsca):
    """layer.py:1285-1290, 1330-1335: the FITS truth and labnoise files of ``L2_2506`` are flipped, along x for SCAs 3, 6, ..., else along y."""
    if informat != "L2_2506":
        return FLIP_NONE
    return FLIP_X if int(idsca[1]) % 3 == 0 else FLIP_Y


def _source(data, dev):
    """(the device tensor the entry reads, type code, swapped, shape) of a source image: a numpy array of either byte order and any strides
    (the bytes go up as they are; a non-contiguous one is made contiguous on the host first), or a tensor on the device."""
    import torch

    if is_torch(data):
        if not data.is_cuda:
            return _source(data.numpy(), dev)
        name = str(data.dtype).replace("torch.", "")
        if name not in SOURCE_TYPES or data.dim() != 2:
            raise TypeError(f"build_cube: a source is a 2D image of {sorted(SOURCE_TYPES)}, not {name} with {data.dim()} axes")
        return data.to(dev).contiguous(), SOURCE_TYPES[name], 0, tuple(int(s) for s in data.shape)
    if not isinstance(data, np.ndarray):
        data = np.asarray(data)
    name = data.dtype.newbyteorder("=").name if data.dtype.kind in "fiu" else str(data.dtype)
    if name not in SOURCE_TYPES:
        raise TypeError(f"build_cube: a source is an image of {sorted(SOURCE_TYPES)}, not {data.dtype}")
    if data.ndim != 2:
        raise ValueError(f"build_cube: a source of shape {data.shape} is no [ny, nx] image")
    data = np.ascontiguousarray(data)  # (keeps the byte order)
    raw = data.view(np.uint8).reshape(-1)
    with warnings.catch_warnings():  # a memory-mapped FITS image is read-only; it is only read
        warnings.simplefilter("ignore", UserWarning)
        raw_d = torch.from_numpy(raw).to(dev)
    return raw_d, SOURCE_TYPES[name], 0 if data.dtype.isnative else 1, data.shape


def place(data, dst, *, origin=(0, 0), flip=FLIP_NONE, subtract=None, scale=None, ctx=None):
    """``dst`` (a contiguous float32 plane [nside, nside] of a cube on the device) = the window of ``data`` at ``origin`` = (y0, x0), flipped,
    minus ``subtract`` and times ``scale`` where given, in numpy's arithmetic (imcom_layer_place)."""
    nside = int(dst.shape[-1])
    src, code, swapped, shape = _source(data, dst.device)
    ctx = bound_context(dst.device, ctx)
    check(lib.imcom_layer_place(ctx.handle, ptr(src), code, swapped, int(shape[0]), int(shape[1]), int(origin[0]), int(origin[1]), int(flip),
                                0 if subtract is None else 1, 0.0 if subtract is None else float(subtract), 0 if scale is None else 1,
                                0.0 if scale is None else float(scale), ptr(dst), nside, MEM_DEVICE))
    return dst


def _split(got):
    """(array, subtract) of what ``sources`` returned."""
    if isinstance(got, tuple):
        return got[0], (None if got[1] is None else float(got[1]))
    return got, None


def _exact(data, nside, what):
    shape = tuple(int(s) for s in np.shape(data))
    if shape != (nside, nside):
        raise ValueError(f"build_cube: the {what} source has shape {shape}, the plane is ({nside}, {nside})")


def _labnoise_origin(data, nside):
    """layer.py:1321-1324: the whole image when it has the plane's shape, else the literal slice [4:4092, 4:4092], which must then have it."""
    shape = tuple(int(s) for s in np.shape(data))
    if shape == (nside, nside):
        return (0, 0)
    if len(shape) == 2:
        cut = tuple(max(0, min(4092, n) - 4) for n in shape)
        if cut == (nside, nside):
            return (4, 4)
        raise ValueError(f"could not broadcast input array from shape {cut} into shape ({nside}, {nside})")
    raise ValueError(f"build_cube: the labnoise source has shape {shape}, the plane is ({nside}, {nside})")


def _default_galsim(cfg_like, idsca, inwcs, inpsf, obsdata, nside):
    """The reference's own GalSimInject calls (layer.py:1391-1456) on the host.  UNVERIFIED: galsim is not installed where this is built."""

    def provider(name, i):
        try:
            from pyimcom.layer import GalSimInject  # the reference package; it imports galsim
        except ImportError as e:
            raise ImcomError(IMCOM_ERR_UNSUPPORTED, f"layer {name!r} (extrainput[{i}]) is drawn by GalSim, which cannot be imported ({e}); "
                             "pass galsim_layers= to build_cube") from None
        kind, oversamp = galsim_kind(name), cfg_like.inpsf_oversamp
        m = re.search(dict(GALSIM_TESTS)[kind], name, re.IGNORECASE)
        res = int(m.group(1))
        if kind == "gsstar":
            return GalSimInject.galsim_star_grid(res, inwcs, inpsf, idsca, obsdata, nside, oversamp)
        if kind == "gstrstar":
            return GalSimInject.galsim_star_grid(res, inwcs, inpsf, idsca, obsdata, nside, oversamp, extraargs={"angleTransient": True})
        if kind == "gsfdstar":
            return GalSimInject.galsim_star_grid(res, inwcs, inpsf, idsca, obsdata, nside, oversamp, extraargs={"FieldDependentModulation": float(m.group(2))})
        if kind == "gsext":
            return GalSimInject.galsim_extobj_grid(res, inwcs, inpsf, nside, oversamp, extraargs=name.split(",")[1:])
        chrom_inpsf = GalSimInject.get_psf(name.split(",")[1], idsca)
        return GalSimInject.galsim_extobj_grid(res, inwcs, chrom_inpsf, nside, oversamp, extraargs=name.split(",")[2:], chrom=True)

    return provider


def build_cube(cfg_like, idsca, sources, *, inwcs=None, inpsf=None, obsdata=None, star_grid=None, grid_image=None, galsim_layers=None, nside=None,
               device=DEVICE, ctx=None):
    """The cube of ``get_all_data`` (layer.py:1252-1492) as a float32 tensor [n_inframe, nside, nside] on ``device``.

    ``cfg_like``: ``n_inframe, extrainput, informat, inpsf_oversamp``.  ``sources(kind, label=None)`` with kind "sci", "truth", "labnoise",
    "skyerr" or "noise" returns None (a missing file: the plane stays zero), an image or ``(image, subtract)`` with the ``float(SKY_MEAN)``
    of 1261 / 1344; for "noise" it returns the slice already chosen (``pick_noise_slice``).  An image is numpy (f4, f8, i2, u2, i4, u1,
    either byte order, any strides) or a tensor on the device; anything else raises TypeError.  ``grid_image(res)`` replaces
    ``inject.make_image_from_grid_device`` (float64, a device tensor or numpy); ``galsim_layers(name, i)`` returns the host image of a GalSim layer
    (default: the reference's GalSimInject; without GalSim ``ImcomError`` of status unsupported, never a zero plane).

    The loop is the reference's: plane 0 is the science frame; ``extrainput[i]`` is tried against every test in the reference's order and a
    later match overwrites an earlier one; a name that matches nothing and a missing source leave zeros.  One brightness image per ``res``
    is made per cube and shared by ``cstar`` and ``nstar``."""
    import torch

    from . import inject, noiselayers
    from .simmask import _sca_nside

    dev = torch.device(device)
    nside = _sca_nside() if nside is None else int(nside)
    n_inframe, extrainput, informat = int(cfg_like.n_inframe), cfg_like.extrainput, cfg_like.informat
    idsca = (int(idsca[0]), int(idsca[1]))
    cube = torch.zeros((n_inframe, nside, nside), dtype=torch.float32, device=dev)
    flip = flip_of(informat, idsca)
    images = {}  # res -> the float64 brightness on the device

    def brightness(res):
        if res not in images:
            if grid_image is not None:
                img = grid_image(res)
            else:
                img = inject.make_image_from_grid_device(res, inpsf, idsca, obsdata, inwcs, nside, cfg_like.inpsf_oversamp, star_grid=star_grid)
            if not is_torch(img):
                img = torch.from_numpy(np.ascontiguousarray(img, dtype=np.float64))
            if img.dtype != torch.float64 or tuple(img.shape) != (nside, nside):
                raise TypeError(f"build_cube: the star image of res {res} is float64 [{nside}, {nside}], not {img.dtype} {tuple(img.shape)}")
            images[res] = img.to(dev).contiguous()
        return images[res]

    # plane 0 (1256-1264)
    if informat in FITS_FORMATS + ASDF_FORMATS:
        data, sub = _split(sources("sci"))
        if data is not None:
            _exact(data, nside, "sci")
            place(data, cube[0], subtract=sub if informat in FITS_FORMATS else None, ctx=ctx)

    for i in range(1, n_inframe):
        name = extrainput[i]
        # truth (1272-1295)
        if name.casefold() == "truth".casefold() or name[:6].casefold() == "truth,".casefold():
            rescale = 1.0
            m = re.search(r"^truth,(.+)$", name, re.IGNORECASE)
            if m:
                rescale = float(m.group(1))
            data, _ = _split(sources("truth"))
            if data is not None:
                _exact(data, nside, "truth")
                place(data, cube[i], flip=flip, scale=rescale, ctx=ctx)
        # white noise (1298-1305)
        m = re.search(r"^whitenoise(\d+)$", name, re.IGNORECASE)
        if m:
            place(noiselayers.white_noise_frame(layer_seed(int(m.group(1)), idsca), nside, device=dev), cube[i], ctx=ctx)
        # 1/f noise (1308-1313)
        m = re.search(r"^1fnoise(\d+)$", name, re.IGNORECASE)
        if m:
            if nside != 4088:
                raise ValueError(f"build_cube: {name!r} is a [4088, 4088] frame (layer.py:913), the cube's nside is {nside}")
            with torch.cuda.device(dev):
                cube[i].copy_(noiselayers.noise_1f_frame(layer_seed(int(m.group(1)), idsca), device_out=True))
        # lab noise (1316-1337)
        if name.casefold() == "labnoise".casefold():
            data, _ = _split(sources("labnoise"))
            if data is not None:
                place(data, cube[i], origin=_labnoise_origin(data, nside), flip=flip, ctx=ctx)
            else:
                print("Warning: labnoise file not found, skipping ...")
        # skyerr (1340-1344)
        if name.casefold() == "skyerr".casefold():
            data, sub = _split(sources("skyerr"))
            if data is not None:
                _exact(data, nside, "skyerr")
                place(data, cube[i], subtract=sub, ctx=ctx)
        # star grid (1347-1353)
        m = re.search(r"^cstar(\d+)$", name, re.IGNORECASE)
        if m:
            place(brightness(int(m.group(1))), cube[i], ctx=ctx)
        # noisy star grid (1357-1388)
        if re.search(r"^nstar(\d+),", name, re.IGNORECASE):
            res, tot_int, bg, q = inject.parse_nstar(name)
            cube[i].copy_(inject.nstar_layer(brightness(res), tot_int, bg, q, idsca, device_out=True))
        # GalSim layers (1391-1456)
        if galsim_kind(name) is not None:
            provider = galsim_layers or _default_galsim(cfg_like, idsca, inwcs, inpsf, obsdata, nside)
            data = provider(name, i)
            _exact(data, nside, name)
            place(data, cube[i], ctx=ctx)
        # saved noise realisations (1460-1490)
        m = re.search(r"^noise,(\S+)", name, re.IGNORECASE)
        if m:
            data, _ = _split(sources("noise", str(m.group(1))))
            if data is not None:
                _exact(data, nside, name)
                place(data, cube[i], ctx=ctx)
    return cube


class FileSources:
    """``sources`` of ``build_cube`` from the reference's files: the statements layer.py:1256-1264, 1280-1293, 1317-1324, 1341-1344 and
    1463-1490 with the reference's own ``_get_sca_imagefile``, astropy and asdf, imported on first use.  An image is handed on as the file
    holds it (a FITS image big-endian, copied out of the file's map and not converted).  UNVERIFIED: none of the three is installed where
    this library is built."""

    def __init__(self, inimage):
        cfg = inimage.blk.cfg
        self.path, self.idsca, self.obsdata, self.informat = cfg.inpath, inimage.idsca, inimage.blk.obsdata, cfg.informat

    def filename(self, kind):
        from os.path import exists

        from pyimcom.layer import _get_sca_imagefile

        extra = {} if kind == "sci" else {"extraargs": {"type": kind}}
        name = _get_sca_imagefile(self.path, self.idsca, self.obsdata, self.informat, **extra)
        return name, exists(name)

    def __call__(self, kind, label=None):
        name, there = self.filename(kind)
        if kind == "labnoise":
            print("lab noise: searching for " + name)
        if kind == "noise":
            print("extracting noise layer " + label + " from " + name)
            if not there:
                warnings.warn("WARNING: cannot find noise file: " + name + ": continuing")
        if not there:
            return None
        if kind == "noise" or (kind == "sci" and self.informat in ASDF_FORMATS) or (kind == "truth" and name[-5:] == ".asdf"):
            import asdf

            with asdf.open(name) as f:
                if kind != "noise":
                    return np.array(f["roman"]["data"])
                jn = pick_noise_slice(f["config"]["NOISE"]["LAYER"], label, name)
                return None if jn < 0 else np.array(f["noise"][jn, :, :])
        from astropy.io import fits

        with fits.open(name) as f:
            if kind == "sci":
                return np.array(f["SCI"].data), float(f["SCI"].header["SKY_MEAN"])
            if kind == "skyerr":
                return np.array(f["ERR"].data), float(f["SCI"].header["SKY_MEAN"])
            return np.array(f[0].data)  # truth, labnoise


def _cache_paths(inimage):
    idsca = inimage.idsca
    path = inimage.blk.cfg.inlayercache + f"_{idsca[0]:08d}_{idsca[1]:02d}.fits"
    return path, path + ".lock"


def load_cached_file(inimage):
    """layer.py:1240-1250: the cube of ``cfg.inlayercache`` under its lock file, float32, or None.  UNVERIFIED (astropy, filelock)."""
    from os.path import exists

    from astropy.io import fits
    from filelock import FileLock, Timeout

    path, lockpath = _cache_paths(inimage)
    try:
        with FileLock(lockpath).acquire(timeout=30):
            if exists(path):
                print("loading input layer <<", path)
                with fits.open(path) as f:
                    return f[0].data.astype(np.float32)
    except Timeout:
        pass
    return None


def save_cached_file(inimage, host_cube):
    """layer.py:1496-1527: write the cube and the science WCS beside it, unless the file is there.  UNVERIFIED (astropy, asdf, filelock)."""
    from os.path import exists

    import asdf
    from astropy.io import fits
    from filelock import FileLock, Timeout
    from pyimcom.wcsutil import PyIMCOM_WCS

    path, lockpath = _cache_paths(inimage)
    nside = int(host_cube.shape[-1])
    try:
        with FileLock(lockpath).acquire(timeout=1):
            if exists(path):
                return
            print("saving input layer >>", path)
            pr = fits.PrimaryHDU(host_cube)
            inwcs = inimage.inwcs
            if isinstance(inwcs, PyIMCOM_WCS):
                if inwcs.constructortype == "GWCS":  # the gwcs goes into an ASDF file beside the cube
                    sciwcs = fits.ImageHDU()
                    sciwcs.header["WCSTYPE"] = "GWCS"
                    fits.HDUList([pr, sciwcs]).writeto(path)
                    af = asdf.AsdfFile()
                    af["wcs"] = inwcs.obj
                    af.write_to(path[:-5] + "_wcs.asdf")
                    return
                inwcs = inwcs.obj
            sciwcs = fits.ImageHDU(np.zeros((nside, nside), dtype=np.uint8), header=inwcs.to_header(relax=True), name="SCIWCS")
            sciwcs["WCSTYPE"] = "FITS"  # (as layer.py:1526 has it)
            fits.HDUList([pr, sciwcs]).writeto(path)
    except Timeout:
        pass


def get_all_data(inimage, device_out=False, *, sources=None, load_cached=load_cached_file, save_cached=save_cached_file, cache=None, **kw):
    """``pyimcom.layer.get_all_data(inimage)`` (layer.py:1199-1527) with the reference's signature: sets ``inimage.indata`` to the float32
    cube, a numpy array, or with ``device_out`` the tensor on the device that ``simmask.load_cr_mask`` and ``inpool`` take as it is.
    ``sources``: ``FileSources(inimage)`` unless given.  ``cfg.inlayercache`` is served by the host hooks ``load_cached(inimage)`` -> cube or
    None and ``save_cached(inimage, host_cube)``; ``cache``: a ``CubeCache`` asked first.  Further keywords go to ``build_cube``."""
    import torch

    cfg = inimage.blk.cfg
    dev = torch.device(kw.get("device", DEVICE))
    use_file_cache = bool(cfg.inlayercache)

    def build():
        if use_file_cache:
            cached = load_cached(inimage)
            if cached is not None:
                return torch.from_numpy(np.ascontiguousarray(cached, dtype=np.float32)).to(dev)
        cube = build_cube(cfg, inimage.idsca, sources if sources is not None else FileSources(inimage), inwcs=inimage.inwcs, inpsf=inimage.get_psf_pos,
                          obsdata=inimage.blk.obsdata, **kw)
        if use_file_cache:
            save_cached(inimage, cube.cpu().numpy())
        return cube

    cube = cache.get(inimage.idsca, build) if cache is not None else build()
    inimage.indata = cube if device_out else cube.cpu().numpy()


class CubeCache:
    """The device twin of ``cfg.inlayercache`` within one process: cubes by (obsid, sca), least recently used first out, ``max_bytes`` in
    all.  Pure Python over torch tensors -- the memory is torch's ("Device memory: one owner"); dropping a cube hands it
    back to torch's allocator."""

    def __init__(self, max_bytes):
        self.max_bytes = int(max_bytes)
        self.bytes = 0
        self._cubes = OrderedDict()

    @staticmethod
    def nbytes(cube):
        return int(cube.numel()) * int(cube.element_size())

    def get(self, idsca, build):
        """The cube of ``idsca``: the cached tensor (now the most recently used), or ``build()``, kept unless it alone exceeds the budget."""
        key = (int(idsca[0]), int(idsca[1]))
        if key in self._cubes:
            self._cubes.move_to_end(key)
            return self._cubes[key]
        cube = build()
        size = self.nbytes(cube)
        if size > self.max_bytes:
            return cube
        while self._cubes and self.bytes + size > self.max_bytes:
            _, old = self._cubes.popitem(last=False)
            self.bytes -= self.nbytes(old)
        self._cubes[key] = cube
        self.bytes += size
        return cube

    def keys(self):
        return list(self._cubes)

    def __len__(self):
        return len(self._cubes)

    def clear(self):
        self._cubes.clear()
        self.bytes = 0
