"""A block's input-stamp pool built on the device from two WCSs (seam 17): what the reference does between reading an exposure and handing
its pixels to the output stamps -- ``InImage.partition_pixels`` (src/pyimcom/coadd.py:174-380), ``InImage.extract_layers`` (382-408) and
``InStamp.__init__`` (682-707), driven by ``Block.process_input_images``.  The binding (seam 17):

    part = pyimcom_amd.inpool.partition_image(inimage.inwcs, blk.outwcs, blk.use_instamps, cfg.n2, cfg.n1P, npixmax, mask=mask)
    inimage.data = part.extract_layers(indata)                       # in place of partition_pixels / extract_layers

    pb = pyimcom_amd.inpool.PoolBuilder(blk.outwcs, blk.use_instamps, cfg.n2, cfg.n1P, npixmax, cfg.n_inframe)
    for inwcs, indata, mask in exposures:
        pb.add_image(inwcs, indata, mask)                            # False: irrelevant, takes no exposure index (coadd.py:1905-1906)
    pool, pix_cumsum = pb.finish()                                   # the select.InStampPool that refblock reads

Only the (sp_res + 1)^2 nodes of the sparse grid are looked at on the host (their positions come from the device's ``wcs._pix2pix``); no
per-pixel work is done and no per-pixel array exists there.  csrc/partition.hip decodes a visit index to its pixel from a prefix sum over
the relevant cells (csrc/partition_core.h), forms the pixel's position with csrc/wcs_core.h's ``wcs_pix2pix`` -- the same bits as
``imcom_wcs_pix2pix`` on the same integer pixel --, and partitions stably by stamp with the radix sort of that file.

Agreement of the positions with astropy is inherited from seam 16 (pyimcom_amd/wcs.py) and is still unchecked: astropy is not installed where
this is built and tested.  What stays on the host: FITS / ASDF, the permanent and file masks (their product is passed in), ``get_psf_pos``,
the visualisation branches.  The layer cube ``indata`` comes from the device as well: ``layers.get_all_data(inimage, device_out=True)``
(seam 23) builds it there and only the file bytes are uploaded; the cosmic-ray mask is seam 10's."""

import ctypes as C

import numpy as np

from . import wcs as _wcs
from ._dev import DEVICE, bound_context
from ._lib import check, lib, ptr
from .select import InStampPool

__all__ = ["relevant_cells", "npixmax_of", "partition_image", "Partition", "PoolBuilder"]

_ARCSEC = 4.84813681109536e-06  # Settings.arcsec (config.py:87)


def _limits(n2, n1P):
    return -n2 - 0.5, n1P * n2 + n2 - 0.5  # coadd.py:207-208 (NsideP = n1P n2)


def _relevance(sp_outxys, use_instamps, n2, n1P):
    """The loop of coadd.py:210-233 on the node positions sp_outxys [2, sp_res + 1, sp_res + 1]: only the interior nodes vote; a node in range
    whose clipped 5 x 5 stamp window holds a stamp in use marks its clipped 5 x 5 cell window.  (is_relevant, relevant_matrix)."""
    sp_outxys = np.asarray(sp_outxys, dtype=np.float64)
    sp_res = sp_outxys.shape[1] - 1
    use = np.asarray(use_instamps, dtype=bool)
    nst = n1P + 2
    pix_lower, pix_upper = _limits(n2, n1P)
    x, y = sp_outxys[0], sp_outxys[1]
    with np.errstate(invalid="ignore"):
        inr = (pix_lower < x) & (x < pix_upper) & (pix_lower < y) & (y < pix_upper)
    inr[0, :] = inr[-1, :] = inr[:, 0] = inr[:, -1] = False
    is_relevant = False
    matrix = np.zeros((sp_res, sp_res), dtype=bool)
    for j, i in zip(*np.nonzero(inr)):
        i_st, j_st = int((x[j, i] - pix_lower) // n2), int((y[j, i] - pix_lower) // n2)
        if np.any(use[max(j_st - 2, 0):min(j_st + 3, nst), max(i_st - 2, 0):min(i_st + 3, nst)]):
            is_relevant = True
            matrix[max(j - 2, 0):min(j + 3, sp_res), max(i - 2, 0):min(i + 3, sp_res)] = True
    return is_relevant, matrix


def relevant_cells(inwcs, outwcs, use_instamps, n2, n1P, nside=_wcs.SCA_NSIDE, sp_res=90, device=DEVICE, ctx=None):
    """The sparse grid of coadd.py:200-233: (is_relevant, relevant_matrix bool [sp_res, sp_res], sp_arr uint16 [sp_res + 1]).  The
    (sp_res + 1)^2 node positions come from the device; the relevance loop runs on the host."""
    a, b = _wcs.as_device_wcs(inwcs), _wcs.as_device_wcs(outwcs)
    sp_arr = np.linspace(0, nside, sp_res + 1, dtype=np.uint16)
    gx, gy = np.meshgrid(sp_arr.astype(np.float64), sp_arr.astype(np.float64))
    x, y, _, _ = _wcs._pix2pix(a, b, points=np.stack((gx.ravel(), gy.ravel()), axis=1), nside=nside, want="x", device=device, ctx=ctx)
    nodes = np.stack((x.cpu().numpy(), y.cpu().numpy())).reshape(2, sp_res + 1, sp_res + 1)
    is_relevant, matrix = _relevance(nodes, use_instamps, n2, n1P)
    return is_relevant, matrix, sp_arr


def npixmax_of(n2, dtheta_deg, pixscale_arcsec=0.11, relax_coef=1.05):
    """The most input pixels of one image that a stamp is given room for (coadd.py:267-275), with the reference's own roundings."""
    return int(((n2 * dtheta_deg * 3600.0) / ((pixscale_arcsec * _ARCSEC) / _ARCSEC) + 1) ** 2 * relax_coef)


class Partition:
    """What ``InImage.partition_pixels`` leaves on an InImage: ``is_relevant``; for a relevant image ``y_idx``, ``x_idx`` (uint16), ``y_val``,
    ``x_val`` (float64) [nst, nst, npixmax] and ``pix_count`` (uint32) [nst, nst] as tensors on the device, ``max_count`` (int), and the
    inputs of the launch (``relevant_matrix``, ``sp_arr``, ``n_visited``).  An irrelevant image holds nothing on the device."""

    def __init__(self, is_relevant, relevant_matrix, sp_arr, nside, ctx=None):
        self.is_relevant, self.relevant_matrix, self.sp_arr, self.nside, self._ctx = is_relevant, relevant_matrix, sp_arr, int(nside), ctx
        self.y_idx = self.x_idx = self.y_val = self.x_val = self.pix_count = None
        self.pix_count_host = None
        self.max_count = 0
        self.n_visited = 0

    def numpy(self):
        """dict of numpy arrays under the reference's attribute names, for its consumers."""
        out = {"is_relevant": self.is_relevant, "max_count": self.max_count}
        if self.is_relevant:
            out.update({k: getattr(self, k).cpu().numpy() for k in ("y_idx", "x_idx", "y_val", "x_val")}, pix_count=self.pix_count_host.copy())
        return out

    def extract_layers(self, indata):
        """``InImage.extract_layers`` (coadd.py:394-404): data float32 [n_inframe, nst, nst, max_count] on the device from ``indata``
        [n_inframe, nside, nside] (a float32 tensor on the device, or numpy)."""
        import torch

        if not self.is_relevant:
            raise ValueError("inpool: extract_layers of an image that is not relevant to the block")
        dev = self.y_idx.device
        if not torch.is_tensor(indata):
            from .stamps import h2d

            indata = h2d(indata, dev, np.float32)
        indata = indata.to(dev, torch.float32).contiguous()
        if indata.dim() != 3 or tuple(indata.shape[1:]) != (self.nside, self.nside):
            raise ValueError(f"inpool: input layers of shape {tuple(indata.shape)}, expected (n_inframe, {self.nside}, {self.nside})")
        nst = self.pix_count.shape[0]
        data = torch.empty((indata.shape[0], nst, nst, self.max_count), dtype=torch.float32, device=dev)
        ctx = bound_context(dev, self._ctx)
        check(lib.imcom_extract_layers(ctx.handle, ptr(indata), indata.shape[0], self.nside, ptr(self.y_idx), ptr(self.x_idx), ptr(self.pix_count), nst * nst,
                                       self.y_idx.shape[2], self.max_count, ptr(data)))
        return data


def _device_mask(mask, nside, dev):
    import torch

    if mask is None:
        return None
    if torch.is_tensor(mask):
        m = mask.to(dev)
        m = m if m.dtype == torch.uint8 else m.to(torch.bool).to(torch.uint8)
    else:
        from .stamps import h2d

        m = h2d(np.asarray(mask).astype(bool).view(np.uint8), dev)
    if tuple(m.shape) != (nside, nside):
        raise ValueError(f"inpool: a frame mask of shape {tuple(m.shape)}, expected ({nside}, {nside})")
    return m.contiguous()


def partition_image(inwcs, outwcs, use_instamps, n2, n1P, npixmax, mask=None, nside=None, sp_res=90, device=DEVICE, ctx=None):
    """``InImage.partition_pixels`` (coadd.py:200-233 and 329-358) with the positions formed on the device.  ``inwcs`` / ``outwcs``: anything
    ``wcs.as_device_wcs`` takes; ``mask``: the frame mask [nside, nside] (true = good) as numpy or as the uint8 device tensor ``simmask``
    returns, None for none.  Returns a ``Partition``; ImcomError where a stamp would receive more than ``npixmax`` pixels."""
    import torch

    a, b = _wcs.as_device_wcs(inwcs), _wcs.as_device_wcs(outwcs)
    nside = int(a.array_shape[-1] if nside is None else nside)
    dev = torch.device(device)
    is_relevant, matrix, sp_arr = relevant_cells(a, b, use_instamps, n2, n1P, nside=nside, sp_res=sp_res, device=dev, ctx=ctx)
    part = Partition(is_relevant, matrix, sp_arr, nside, ctx)
    if not is_relevant:
        return part
    nst = n1P + 2
    use = np.ascontiguousarray(np.asarray(use_instamps).astype(bool).view(np.uint8))
    if use.shape != (nst, nst):
        raise ValueError(f"inpool: use_instamps of shape {use.shape}, expected ({nst}, {nst})")
    use_d = torch.as_tensor(use, device=dev)
    mk = _device_mask(mask, nside, dev)
    part.y_idx = torch.zeros((nst, nst, npixmax), dtype=torch.uint16, device=dev)
    part.x_idx = torch.zeros_like(part.y_idx)
    part.y_val = torch.zeros((nst, nst, npixmax), dtype=torch.float64, device=dev)
    part.x_val = torch.zeros_like(part.y_val)
    part.pix_count = torch.zeros((nst, nst), dtype=torch.uint32, device=dev)
    pix_lower, pix_upper = _limits(n2, n1P)
    ctx = bound_context(dev, ctx)
    ta, tb = a._table_args(dev), b._table_args(dev)
    rel = np.ascontiguousarray(matrix.view(np.uint8))
    nvis = C.c_long(0)
    check(lib.imcom_partition_wcs(ctx.handle, ptr(a.descriptor), ta[0], ta[1], ta[2], ta[3], ta[4], ptr(b.descriptor), tb[0], tb[1], tb[2], tb[3], tb[4], ptr(sp_arr),
                                  ptr(rel), int(sp_res), nside, ptr(mk), ptr(use_d), nst, int(n2), pix_lower, pix_upper, int(npixmax), ptr(part.y_idx),
                                  ptr(part.x_idx), ptr(part.y_val), ptr(part.x_val), ptr(part.pix_count), C.byref(nvis)))
    part.n_visited = int(nvis.value)
    part.pix_count_host = part.pix_count.cpu().numpy()
    part.max_count = int(part.pix_count_host.max())
    return part


def _ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _assemble(ctx, lists, counts, xy_pitch, data_pitch, frame_stride, n_inframe, dev, with_expo):
    """imcom_pool_assemble over ``lists`` = [(x, y, data)] with the count table ``counts`` uint32 [n_img, nstamps]: (x, y, data, expo, inst_off)."""
    import torch

    n_img, nstamps = counts.shape
    npool = int(counts.sum(dtype=np.int64))
    x = torch.empty(npool, dtype=torch.float64, device=dev)
    y = torch.empty_like(x)
    data = torch.empty((n_inframe, npool), dtype=torch.float32, device=dev)
    expo = torch.empty(npool, dtype=torch.int32, device=dev) if with_expo else None
    inst_off = torch.empty(nstamps + 1, dtype=torch.int64, device=dev)
    long_arr = lambda v: np.ascontiguousarray(v, dtype=np.int64)  # noqa: E731
    xyp, dp, fs = long_arr(xy_pitch), long_arr(data_pitch), long_arr(frame_stride)
    ex = np.arange(n_img, dtype=np.int32)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    check(lib.imcom_pool_assemble(ctx.handle, n_img, nstamps, n_inframe, _ptr_array([t[0] for t in lists]), _ptr_array([t[1] for t in lists]),
                                  _ptr_array([t[2] for t in lists]), ptr(xyp), ptr(dp), ptr(fs), ptr(ex), ptr(counts), npool, ptr(x), ptr(y), ptr(data), ptr(expo),
                                  ptr(inst_off)))
    return x, y, data, expo, inst_off


class PoolBuilder:
    """The InStamps of a block (coadd.py:682-707 for every stamp at once) from its exposures, on the device.

    ``add_image`` partitions one exposure, gathers its layers and keeps the result as COMPACT stamp-major lists -- x, y float64 [T],
    data float32 [n_inframe, T] with T the image's kept pixels, and the counts uint32 [nst^2] on the host -- not the npixmax-padded arrays.
    ``finish`` lays the lists out stamp by stamp, the images of a stamp in list order, with one segmented copy (no sort).

    Device bytes.  With S = nst^2 stamps, F = n_inframe, V the pixels an image visits, T_m the kept pixels of image m, npool = sum T_m and
    M the relevant images:
      * held between calls: (16 + 4 F) T_m for every image added so far;
      * inside ``add_image`` in addition: the padded arrays 20 S npixmax + 4 S, the layers 4 F S max_count, the frame mask nside^2 if it came
        as numpy, 8 (S + 1) for the offsets, and the library's workspace of 16 (V + 1) + 256 ceil(V / 2048) + 16 + 4 (S + 1) + 4 +
        8 (cells + 1) + 2 (sp_res + 1) bytes (each of its ten buffers rounded up to 256), beside the caller's own 4 F nside^2 of layers;
      * inside ``finish`` in addition: the pool (20 + 4 F) npool + 8 (S + 1), and a workspace of 28 M S + 36 M bytes.
    The peak of a block is therefore (16 + 4 F) npool + max(the ``add_image`` terms of the last image, the ``finish`` terms): for a 48 x 48-stamp
    block (S = 2500) of 4088^2 exposures, F = 4, npixmax = 168, V = 4088^2, that is 32 npool + about 0.29 GB inside ``add_image`` -- the sort's 16 bytes
    a visited pixel -- against (32 + 36) npool inside ``finish``."""

    def __init__(self, outwcs, use_instamps, n2, n1P, npixmax, n_inframe, nside=None, sp_res=90, device=DEVICE, ctx=None):
        self.outwcs = _wcs.as_device_wcs(outwcs)
        self.use_instamps = np.asarray(use_instamps).astype(bool)
        self.n2, self.n1P, self.npixmax, self.n_inframe = int(n2), int(n1P), int(npixmax), int(n_inframe)
        self.nside, self.sp_res, self.device, self.ctx = nside, int(sp_res), device, ctx
        self.lists, self.counts = [], []

    def add_image(self, inwcs, indata, mask=None):
        """One exposure: its WCS, its layers [n_inframe, nside, nside] and its frame mask.  Returns ``is_relevant``; an irrelevant image is
        dropped and takes no exposure index."""
        part = partition_image(inwcs, self.outwcs, self.use_instamps, self.n2, self.n1P, self.npixmax, mask=mask, nside=self.nside, sp_res=self.sp_res,
                               device=self.device, ctx=self.ctx)
        if not part.is_relevant:
            return False
        data = part.extract_layers(indata)
        if data.shape[0] != self.n_inframe:
            raise ValueError(f"inpool: {data.shape[0]} input layers, the pool holds {self.n_inframe}")
        nst = self.n1P + 2
        counts = part.pix_count_host.reshape(1, nst * nst)
        ctx = bound_context(data.device, self.ctx)
        x, y, d, _, _ = _assemble(ctx, [(part.x_val, part.y_val, data)], counts, [self.npixmax], [part.max_count], [nst * nst * part.max_count], self.n_inframe,
                                  data.device, False)
        self.lists.append((x, y, d))
        self.counts.append(counts[0].copy())
        return True

    def finish(self):
        """(``select.InStampPool``, pix_cumsum uint32 [nst^2, n_img + 1] on the host: ``InStamp.pix_cumsum`` of every stamp)."""
        import torch

        nst = self.n1P + 2
        dev = torch.device(self.device)
        counts = np.array(self.counts, dtype=np.uint32).reshape(len(self.lists), nst * nst)
        ctx = bound_context(dev, self.ctx)
        x, y, data, expo, inst_off = _assemble(ctx, self.lists, counts, [0] * len(self.lists), [0] * len(self.lists), [t[0].numel() for t in self.lists],
                                               self.n_inframe, dev, True)
        pix_cumsum = np.zeros((nst * nst, len(self.lists) + 1), dtype=np.uint32)
        pix_cumsum[:, 1:] = np.cumsum(counts.T, axis=1, dtype=np.uint32)
        return InStampPool.from_device(x, y, data, expo, inst_off, self.n_inframe), pix_cumsum

    def attach(self, blk):
        """``finish()`` and hand the result to ``blk`` for ``refblock.coadd_output_stamps``: ``blk.instamp_pool`` (the pool, left on the device),
        ``blk.n_inimage`` (the relevant exposures) and ``blk.instamps[j][i]`` with what the block seam still reads on the host --
        ``pix_cumsum``, ``pix_count`` and, on the even-even stamps, ``psf_compute_point_pix`` (coadd.py:688-691, 709-712).  Returns the pool."""
        pool, pix_cumsum = self.finish()
        nst = self.n1P + 2
        blk.instamp_pool, blk.n_inimage = pool, len(self.lists)
        blk.instamps = [[None] * nst for _ in range(nst)]
        for j_st in range(nst):
            for i_st in range(nst):
                st = _InStamp()
                st.j_st, st.i_st = j_st, i_st
                st.pix_cumsum = pix_cumsum[j_st * nst + i_st]
                st.pix_count = np.diff(st.pix_cumsum.astype(np.int64)).astype(np.uint32)
                if j_st % 2 == 0 and i_st % 2 == 0:
                    st.psf_compute_point_pix = [i_st * self.n2 - 0.5, j_st * self.n2 - 0.5]
                blk.instamps[j_st][i_st] = st
        return pool


class _InStamp:
    """The host side of an InStamp whose pixels live in the pool (PoolBuilder.attach)."""
