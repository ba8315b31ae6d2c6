"""HEALPix star grids on the device: the pixels of the RING scheme inside a circle on the sky, their centres, and those centres through a
WCS -- what every injected-star path of the reference starts from.  ``GridInject.make_sph_grid`` / ``generate_star_grid``
(src/pyimcom/layer.py:690-789) and the ``healpy.ang2vec`` + ``query_disc`` + ``pix2ang`` + ``all_world2pix`` + box selection of
``StarsAnal.__call__`` (analysis.py:957-978), ``gen_starcube_nonoise`` (starcube_nonoise.py:145-175), ``gen_dynrange_data``
(dynrange.py:167-191) and ``gen_truthcats`` (truthcats.py:190-241).  The binding (seam 18):

    image = pyimcom_amd.inject.make_image_from_grid(res, inpsf, idsca, obsdata, mywcs, nside, oversamp,
                                                    star_grid=pyimcom_amd.healpix.generate_star_grid)
    g = pyimcom_amd.healpix.block_star_grid(res, block_header, n, bdpad, search_radius)    # ipix, ra, dec, x, y, xi, yi (, pa)

csrc/wcs.hip gives every ring of the cap one workgroup (count, scan, fill: ascending pixels, no atomics); csrc/healpix_core.h holds the
arithmetic.  healpy and the reference package are not needed.

WHAT IS VERIFIED AND WHAT IS NOT.  healpy is not installed where this code is built and tested.  The arithmetic is that of Gorski et al. 2005
(ApJ 622, 759: section 4.1, eqs. 2-9, and the inverse), and the device is compared with those definitions evaluated in 40-digit arithmetic
(tests/healpix_reference.py, tests/golden/make_golden_healpix.py).  Agreement with healpy itself has NOT been checked; tests/test_healpix_host.py
holds that comparison behind ``pytest.importorskip("healpy")``.  A pixel whose centre lies within a few 1e-16 (in the cosine of the distance)
of the circle may fall on either side, here as in any float64 evaluation.

Served: RING order, ``nside`` = 2^res with res 0 .. 29, int64 pixels.  Refused (``ImcomError``, IMCOM_ERR_UNSUPPORTED): ``nest=True``,
``inclusive=True``, an ``nside`` that is no power of two.

``make_sph_grid`` keeps the reference's pixel range ``pmin .. pmax`` (layer.py:721-725): a cap that holds a pole loses the pixels of the
polar ring beyond ``pmax`` (or before ``pmin``).  ``query_disc`` and ``block_star_grid`` take the full disc.

A numpy input gives numpy results; ``device_out=True`` or tensor inputs give tensors that stay on the device."""

import ctypes as C

import numpy as np

from ._dev import DEVICE, bound_context, device_of, is_torch, staged
from ._lib import MEM_DEVICE, ImcomError, check, lib, ptr
from .wcs import as_device_wcs

__all__ = ["pix2ang", "ang2pix", "ang2vec", "vec2ang", "query_disc", "make_sph_grid", "generate_star_grid", "block_star_grid", "cap", "MAX_RES"]

IMCOM_ERR_UNSUPPORTED = -4
MAX_RES = 29
RANGE_REFERENCE, RANGE_DISC = 0, 1  # the `mode` of imcom_healpix_cap


def _unsupported(msg):
    return ImcomError(IMCOM_ERR_UNSUPPORTED, "healpix: " + msg)


def _res(nside):
    n = int(nside)
    if n != nside or n < 1 or n & (n - 1) or n > 1 << MAX_RES:
        raise _unsupported(f"nside = {nside}: served are the powers of two up to 2^{MAX_RES}")
    return n.bit_length() - 1


def _ring_only(nest):
    if nest:
        raise _unsupported("NEST order is not served (RING only)")


def _to_device(a, dtype, device):
    """(contiguous 1-D tensor of ``a`` on the device, its shape, whether ``a`` was a tensor)."""
    import torch

    was = is_torch(a)
    shape = tuple(a.shape) if was else np.shape(a)
    return staged(a, device_of(a, device=device), astype=np.int64 if dtype is torch.int64 else np.float64).reshape(-1), shape, was


def _home(t, shape, stay):
    t = t.reshape(shape)
    if stay:
        return t
    a = t.cpu().numpy()
    return a if shape else a[()]


def pix2ang(nside, ipix, nest=False, lonlat=False, device_out=False, device=DEVICE, ctx=None):
    """``healpy.pix2ang``: the centres (theta, phi) in radians of the pixels, or with ``lonlat`` (lon, lat) in degrees."""
    import torch

    _ring_only(nest)
    res = _res(nside)
    p, shape, was = _to_device(ipix, torch.int64, device)
    ctx = bound_context(p.device, ctx)
    a, b = torch.empty(p.shape, dtype=torch.float64, device=p.device), torch.empty(p.shape, dtype=torch.float64, device=p.device)
    check(lib.imcom_healpix_pix2ang(ctx.handle, res, ptr(p), p.numel(), int(bool(lonlat)), ptr(a), ptr(b), MEM_DEVICE))
    stay = was or device_out
    return _home(a, shape, stay), _home(b, shape, stay)


def ang2pix(nside, theta, phi, nest=False, lonlat=False, device_out=False, device=DEVICE, ctx=None):
    """``healpy.ang2pix``: the pixels that hold (theta, phi) in radians, or with ``lonlat`` (lon, lat) in degrees."""
    import torch

    _ring_only(nest)
    res = _res(nside)
    if not is_torch(theta) and not is_torch(phi):
        theta, phi = np.broadcast_arrays(np.asarray(theta, dtype=np.float64), np.asarray(phi, dtype=np.float64))
    a, shape, was = _to_device(theta, torch.float64, device)
    b = _to_device(phi, torch.float64, a.device)[0].to(a.device)
    if a.shape != b.shape:
        raise ValueError(f"healpix: {a.numel()} and {b.numel()} angles")
    ctx = bound_context(a.device, ctx)
    p = torch.empty(a.shape, dtype=torch.int64, device=a.device)
    check(lib.imcom_healpix_ang2pix(ctx.handle, res, ptr(a), ptr(b), a.numel(), int(bool(lonlat)), ptr(p), MEM_DEVICE))
    return _home(p, shape, was or device_out)


def ang2vec(theta, phi, lonlat=False):
    """``healpy.ang2vec``: unit vectors [..., 3] of (theta, phi) in radians, or with ``lonlat`` of (lon, lat) in degrees."""
    if lonlat:
        theta, phi = np.pi / 2.0 - np.radians(phi), np.radians(theta)
    theta, phi = np.broadcast_arrays(np.asarray(theta, dtype=np.float64), np.asarray(phi, dtype=np.float64))
    st = np.sin(theta)
    return np.stack((st * np.cos(phi), st * np.sin(phi), np.cos(theta)), axis=-1)


def vec2ang(vectors, lonlat=False):
    """``healpy.vec2ang``: (theta, phi) in radians, phi in [0, 2 pi), or with ``lonlat`` (lon, lat) in degrees."""
    v = np.asarray(vectors, dtype=np.float64).reshape(-1, 3)
    theta = np.arctan2(np.hypot(v[:, 0], v[:, 1]), v[:, 2])
    phi = np.arctan2(v[:, 1], v[:, 0])
    phi = np.where(phi < 0.0, phi + 2.0 * np.pi, phi)
    return (np.degrees(phi), 90.0 - np.degrees(theta)) if lonlat else (theta, phi)


_CAP_FIELDS = ("ipix", "ra", "dec", "ra_deg", "dec_deg", "x", "y", "pa")


def cap(res, ra, dec, radius, full_disc=False, lonlat=False, wcs=None, origin=0, box=None, want=("ipix", "ra", "dec"), device=DEVICE, ctx=None):
    """imcom_healpix_cap: a dict of the device tensors named in ``want`` (of ``ipix, ra, dec, ra_deg, dec_deg, x, y, pa``), ascending in the
    pixel, and "npix".  (ra, dec) and ``radius`` in radians; ``full_disc``: every pixel of the disc instead of the reference's range;
    ``lonlat``: the degrees as healpy's ``lonlat`` forms them instead of rad / (pi / 180); ``wcs``: a DeviceWCS for x, y, pa and the box;
    ``box`` = (n, bdpad): only the pixels with bdpad <= rint(x), rint(y) < n - bdpad.  One counting call, an exact allocation, one filling
    call."""
    import torch

    res = int(res)
    if not 0 <= res <= MAX_RES:
        raise _unsupported(f"res = {res}: served are 0 .. {MAX_RES}")
    unknown = set(want) - set(_CAP_FIELDS)
    if unknown:
        raise ValueError(f"healpix: unknown outputs {sorted(unknown)}")
    dev = torch.device(device)
    ctx = bound_context(dev, ctx)
    desc, tab = None, (None, 0, 0, 0.0, 0.0)
    if wcs is not None:
        desc, tab = wcs.descriptor, wcs._table_args(dev)
    n_box, bdpad = (int(box[0]), int(box[1])) if box is not None else (0, 0)

    def call(capacity, out):
        count = C.c_long(0)
        check(lib.imcom_healpix_cap(ctx.handle, res, float(ra), float(dec), float(radius), RANGE_DISC if full_disc else RANGE_REFERENCE, int(bool(lonlat)), ptr(desc),
                                    tab[0], tab[1], tab[2], tab[3], tab[4], int(origin), n_box, bdpad, capacity, *[ptr(out.get(k)) for k in _CAP_FIELDS],
                                    C.byref(count), MEM_DEVICE))
        return count.value

    n = call(0, {})
    out = {k: torch.empty(n, dtype=torch.int64 if k == "ipix" else torch.float64, device=dev) for k in want}
    if "x" in out or "y" in out:  # (given together)
        for k in ("x", "y"):
            out.setdefault(k, torch.empty(n, dtype=torch.float64, device=dev))
    if n and out:
        call(n, out)
    res_out = {k: out[k] for k in want}
    res_out["npix"] = n
    return res_out


def _host(d, keys):
    return {k: (d[k].cpu().numpy() if k in keys else d[k]) for k in d}


def query_disc(nside, vec, radius, inclusive=False, nest=False, device_out=False, device=DEVICE, ctx=None):
    """``healpy.query_disc``: the ascending pixels whose centres lie within ``radius`` (radians) of the direction ``vec``."""
    _ring_only(nest)
    if inclusive:
        raise _unsupported("inclusive=True is not served (pixel centres only)")
    res = _res(nside)
    theta, phi = vec2ang(vec)
    if len(theta) != 1:
        raise ValueError("healpix: query_disc takes one vector")
    p = cap(res, float(phi[0]), float(np.pi / 2.0 - theta[0]), radius, full_disc=True, want=("ipix",), device=device, ctx=ctx)["ipix"]
    return p if device_out else p.cpu().numpy()


def make_sph_grid(res, ra, dec, radius, device_out=False, device=DEVICE, ctx=None):
    """``GridInject.make_sph_grid`` (layer.py:690-740): the reference's dict, same keys."""
    g = cap(res, ra, dec, radius, device=device, ctx=ctx)
    ipix, rapix, decpix = (g[k] if device_out else g[k].cpu().numpy() for k in ("ipix", "ra", "dec"))
    return {"res": res, "nside": 2**res, "npix": g["npix"], "ipix": ipix, "rapix": rapix, "decpix": decpix}


def generate_star_grid(res, myWCS, scapar={"nside": 4088, "pix_arcsec": 0.11}, device_out=False):
    """``GridInject.generate_star_grid`` (layer.py:743-789): (ipix, px, py, ra, dec in degrees) of the grid points within one SCA side length
    of the SCA's centre.  ``myWCS``: anything ``wcs.as_device_wcs`` takes.  The centre comes from one ``all_pix2world``; the cap, its centres
    and their positions are one device call."""
    w = as_device_wcs(myWCS)
    degree = np.pi / 180
    radius = scapar["nside"] * scapar["pix_arcsec"] / 3600 * degree
    cpos_local = (scapar["nside"] - 1) / 2
    cpos_world = w.all_pix2world([[cpos_local, cpos_local]], 0)[0]
    g = cap(res, cpos_world[0] * degree, cpos_world[1] * degree, radius, wcs=w, want=("ipix", "x", "y", "ra_deg", "dec_deg"))
    out = tuple(g[k] for k in ("ipix", "x", "y", "ra_deg", "dec_deg"))
    return out if device_out else tuple(t.cpu().numpy() for t in out)


def block_star_grid(res, wcs, n, bdpad, search_radius, position_angle=False, device_out=False, device=DEVICE, ctx=None):
    """The statement the four report sites share (analysis.py:957-978, starcube_nonoise.py:145-175, dynrange.py:167-191, truthcats.py:190-241):
    the centre of the block at ((n - 1) / 2, (n - 1) / 2), the disc of ``search_radius`` (radians) about it, the centres in degrees (healpy's
    ``lonlat``), their positions, the selection bdpad <= rint(x), rint(y) < n - bdpad and the int16 ``xi, yi``.  ``wcs``: the block's
    celestial (two-axis) header as a mapping, or a DeviceWCS.  A dict of ``ipix, ra, dec`` (degrees), ``x, y, xi, yi`` and, with
    ``position_angle``, ``pa`` (truthcats.py:229-241)."""
    import torch

    w = as_device_wcs(wcs)
    cen = w.all_pix2world([[(n - 1) / 2, (n - 1) / 2]], 0)[0]
    vec = ang2vec(cen[0], cen[1], lonlat=True)
    theta, phi = vec2ang(vec)
    want = ("ipix", "ra_deg", "dec_deg", "x", "y") + (("pa",) if position_angle else ())
    g = cap(res, float(phi[0]), float(np.pi / 2.0 - theta[0]), search_radius, full_disc=True, lonlat=True, wcs=w, box=(n, bdpad), want=want, device=device, ctx=ctx)
    out = {"ipix": g["ipix"], "ra": g["ra_deg"], "dec": g["dec_deg"], "x": g["x"], "y": g["y"],
           "xi": torch.round(g["x"]).to(torch.int16), "yi": torch.round(g["y"]).to(torch.int16)}
    if position_angle:
        out["pa"] = g["pa"]
    return out if device_out else {k: v.cpu().numpy() for k, v in out.items()}
