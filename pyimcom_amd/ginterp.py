"""The metadetection resampler on the device: a drop-in for ``pyimcom.meta.ginterp`` (reference src/pyimcom/meta/ginterp.py).

``InterpMatrix`` and ``MultiInterp`` keep the reference's signatures, defaults and return types; all arithmetic runs in libimcom_hip
(csrc/ginterp.hip).  numpy in -> numpy out; a torch tensor on the device in -> torch out, with no round trip through the host, so the
shears of one mosaic upload it once.  ``pyimcom.meta.distortimage.ginterp = pyimcom_amd.ginterp`` routes ``MetaMosaic.shearimage`` here
(seam 4)."""

import ctypes as C

import numpy as np

from ._dev import bound_context, is_torch
from ._lib import MEM_DEVICE, MEM_HOST, check, default_context, lib, ptr

__all__ = ["InterpMatrix", "MultiInterp", "geometry", "stest_points"]


def geometry(Rsearch):
    """The grid offsets within the search radius in the reference's order (ginterp.py:62-83) and the corner subsets g_c
    (ginterp.py:157-159): (posx int16 [NN], posy int16 [NN], corners int [4][n_g], indices into posx).  Host code, no device."""
    nn, ng = C.c_int(0), C.c_int(0)
    check(lib.imcom_ginterp_geometry(float(Rsearch), 0, C.byref(nn), C.byref(ng), None, None, None))
    px = np.zeros(nn.value, dtype=np.int32)
    py = np.zeros(nn.value, dtype=np.int32)
    corners = np.zeros((4, ng.value), dtype=np.int32)
    check(lib.imcom_ginterp_geometry(float(Rsearch), nn.value, C.byref(nn), C.byref(ng), ptr(px), ptr(py), ptr(corners)))
    return px.astype(np.int16), py.astype(np.int16), corners


def stest_points(npts, stest=1, blocksize=None):
    """Indices of the points whose U and Sigma the reference evaluates: every stest-th point (InterpMatrix, ginterp.py:175), or, with
    ``blocksize``, every stest-th point of every chunk of MultiInterp's loop (ginterp.py:272-304) -- the points of Umax and Smax."""
    i = np.arange(int(npts))
    return i[(i if blocksize is None else i % int(blocksize)) % int(stest) == 0]


def InterpMatrix(Rsearch, samp, x_out, y_out, Cov, epsilon=1.0e-7, stest=1):
    """``ginterp.InterpMatrix`` (ginterp.py:19-186): returns (posx int16 [NN], posy int16 [NN], T [Npts, NN], U [ceil(Npts/stest)],
    Sigma [ceil(Npts/stest)]), T, U and Sigma float64 (torch tensors on the device if x_out is one)."""
    ctx = default_context()
    posx, posy, _ = geometry(Rsearch)
    nn = posx.size
    cov = np.ascontiguousarray(np.asarray(Cov, dtype=np.float64).ravel()[:3])
    stest = int(stest)
    if is_torch(x_out):
        import torch

        dev = x_out.device
        x = x_out.to(torch.float64).reshape(-1).contiguous()
        y = torch.as_tensor(y_out, device=dev).to(torch.float64).reshape(-1).contiguous()
        n = x.numel()
        nu = (n + stest - 1) // stest
        T = torch.empty((n, nn), dtype=torch.float64, device=dev)
        U = torch.empty(nu, dtype=torch.float64, device=dev)
        S = torch.empty(nu, dtype=torch.float64, device=dev)
        bound_context(ctx=ctx)
        mem = MEM_DEVICE
    else:
        x = np.ascontiguousarray(np.asarray(x_out, dtype=np.float64).ravel())
        y = np.ascontiguousarray(np.asarray(y_out, dtype=np.float64).ravel())
        n = x.size
        nu = (n + stest - 1) // stest
        T = np.empty((n, nn))
        U = np.empty(nu)
        S = np.empty(nu)
        mem = MEM_HOST
    if y.shape[0] != n:
        raise ValueError("x_out and y_out differ in length")
    check(lib.imcom_ginterp_matrix(ctx.handle, float(Rsearch), float(samp), int(n), ptr(x), ptr(y), ptr(cov), float(epsilon), stest, ptr(T), ptr(U),
                                   ptr(S), mem))
    return posx, posy, T, U, S


def MultiInterp(in_array, in_mask, out_size, out_origin, out_transform, Rsearch, samp, Cov, epsilon=1.0e-7, stest=1, blocksize=393216):
    """``ginterp.MultiInterp`` (ginterp.py:189-340): returns (out_array [nlayer,] ny, nx in the input's dtype, out_mask bool [ny, nx],
    Umax, Smax).  2-D in -> 2-D out, 3-D in -> 3-D out; float32 and float64 inputs (others: TypeError)."""
    tor = is_torch(in_array)
    ndim = in_array.ndim
    if ndim not in (2, 3):
        raise ValueError("in_array must be 2-D or 3-D")
    ny, nx = int(out_size[0]), int(out_size[1])
    origin = np.ascontiguousarray(np.asarray(out_origin, dtype=np.float64).ravel()[:2])
    transform = np.ascontiguousarray(np.asarray(out_transform, dtype=np.float64).reshape(2, 2))
    cov = np.ascontiguousarray(np.asarray(Cov, dtype=np.float64).ravel()[:3])
    if tor:
        import torch

        if in_array.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"MultiInterp: in_array dtype {in_array.dtype} (float32 and float64 are supported)")
        dev = in_array.device
        a = in_array.contiguous()
        a3 = a if ndim == 3 else a.unsqueeze(0)
        m = torch.as_tensor(in_mask, device=dev).to(torch.uint8).contiguous()
        nlayer, ny_in, nx_in = a3.shape
        out = torch.empty((nlayer, ny, nx), dtype=a.dtype, device=dev)
        omask = torch.empty((ny, nx), dtype=torch.uint8, device=dev)
        us = torch.empty(2, dtype=torch.float64, device=dev)
        f64 = int(a.dtype == torch.float64)
        mem = MEM_DEVICE
    else:
        a = np.asarray(in_array)
        if a.dtype not in (np.float32, np.float64):
            raise TypeError(f"MultiInterp: in_array dtype {a.dtype} (float32 and float64 are supported)")
        a3 = np.ascontiguousarray(a if ndim == 3 else a[None])
        m = np.ascontiguousarray(np.asarray(in_mask, dtype=bool)).view(np.uint8)
        nlayer, ny_in, nx_in = a3.shape
        out = np.empty((nlayer, ny, nx), dtype=a.dtype)
        omask = np.empty((ny, nx), dtype=np.uint8)
        us = np.zeros(2)
        f64 = int(a.dtype == np.float64)
        mem = MEM_HOST
    if tuple(m.shape) != (ny_in, nx_in):
        raise ValueError(f"in_mask shape {tuple(m.shape)} != {(ny_in, nx_in)}")
    ctx = default_context()
    if tor:
        bound_context(ctx=ctx)
    check(lib.imcom_ginterp_resample(ctx.handle, int(nlayer), int(ny_in), int(nx_in), ptr(a3), f64, ptr(m), ny, nx, ptr(origin), ptr(transform),
                                     float(Rsearch), float(samp), ptr(cov), float(epsilon), int(stest), int(blocksize), ptr(out), ptr(omask),
                                     ptr(us), mem))
    if tor:
        umax, smax = (float(v) for v in us.cpu())
        omask = omask.bool()
    else:
        umax, smax = float(us[0]), float(us[1])
        omask = omask.view(bool)
    return (out if ndim == 3 else out[0]), omask, umax, smax
