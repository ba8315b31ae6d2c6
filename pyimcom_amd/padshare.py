"""Padding stamps shared between neighbouring blocks on the device (seam 20; reference src/pyimcom/analysis.py:394-537,
``OutImage._update_hdu_data``, and 1429-1467, ``Mosaic.share_padding_stamps``; kernels in csrc/block.hip, arithmetic in csrc/padshare_core.h).

With ``pad_sides = "auto"`` a block coadds padding postage stamps only on the mosaic's outer boundary; every interior edge is filled afterwards
from the neighbour.  ``ShareBlock`` is one block as ``_update_hdu_data`` sees it, ``update`` is that method (at most three launches) and
``share_padding_stamps`` the loop, in the reference's order.  FITS reading and writing, the CONFIG HDU with its ``auto -> all`` rewrite and
``Config`` stay the reference's."""

import ctypes as C
import re

import numpy as np
import torch

from ._dev import bound_context
from ._lib import PADSHARE_NO_FLOOR, PadshareMap, check, lib, ptr

DIRECTIONS = ("left", "right", "bottom", "top")
# coadd.py:2247-2305, in the order of hdu_names[5:]: HDU name -> (outmaps letter, BlockMaps name, UNIT value, UNIT comment)
MAP_HDUS = {"FIDELITY": ("U", "UC", "-0.2mB", "-5000*log10(U/C)"), "SIGMA": ("S", "Sigma", "-0.1mB", "-10000*log10(Sigma)"),
            "KAPPA": ("K", "kappa", "-0.2mB", "-5000*log10(kappa)"), "INWTSUM": ("T", "Tsum", "5uB", "200000*log10(Tsum)"),
            "EFFCOVER": ("N", "Neff", "20uB", "50000*log10(Neff)")}


def unit_to_bels(unit, comment):
    """helper.py:19-82, ``HDU_to_bels``: the UNIT value in bels, with the sign fix for legacy files (a positive value whose comment starts
    with '-')."""
    s = re.match(r"([\d\.\-\+eE]+)([mun]?)B", unit)
    if not s:
        return float("nan")
    x = float(s.group(1))
    if s.group(2) == "m":
        x *= 1e-3
    if s.group(2) == "u":
        x *= 1e-6
    if s.group(2) == "n":
        x *= 1e-9
    if x > 0 and comment[:1] == "-":
        x = -x
    return x


def decode_coefficient(unit, comment):
    """analysis.py:377: the double ``1.0 / HDU_to_bels(hdu)`` (200000.00000000003 for "5uB"), not the integer of the comment."""
    return 1.0 / unit_to_bels(unit, comment)


def floor_code(unit, comment, unsigned, zero_floor=None):
    """The code that get_output_map's line 387 turns into 0, or None where it zeroes nothing.  ``a_zero`` is the lowest code for a positive
    coefficient, else the highest.  ``zero_floor=None`` evaluates the reference's own comparison -- a float32 array against a numpy float64
    scalar -- on one element with the installed numpy: numpy >= 2 compares in float64, true only where the power is exactly a float32
    (EFFCOVER's code 0); numpy < 2 demotes the scalar and every floor code is zeroed.  ``True`` / ``False`` force the one or the other."""
    coef = decode_coefficient(unit, comment)
    a_min, a_max = (0, 65535) if unsigned else (-32768, 32767)
    a_zero = a_min if coef > 0 else a_max
    if zero_floor is None:
        data = np.power(10.0, np.array([a_zero]) / coef).astype(np.float32)
        zero_floor = bool((data == np.power(10.0, a_zero / coef))[0])
    return a_zero if zero_floor else None


def idsca_pairs(my_idscas, ur_idscas):
    """analysis.py:468-470: (my_idx, ur_idx) for every (obsid, sca) that both lists hold, each the first occurrence; int32 [npairs, 2]."""
    my, ur = [tuple(x) for x in my_idscas], [tuple(x) for x in ur_idscas]
    return np.array(sorted((my.index(x), ur.index(x)) for x in set(my) & set(ur)), dtype=np.int32).reshape(-1, 2)


class ShareBlock:
    """One block as ``_update_hdu_data`` sees it: ``primary`` float32 [n_out, nlayer, NsideP, NsideP] and ``inweight`` float32
    [n_out, n_inimage, n1P, n1P] on the device, ``idscas`` the (obsid, sca) list of INDATA, ``maps`` a dict HDU name -> (codes (u)int16
    [n_out, NsideP, NsideP] on the device, UNIT value, UNIT comment) in the order of ``hdu_names[5:]``; ``n2``, ``postage_pad`` and
    ``fk = fade_kernel`` are what the method reads from its ``cfg``."""

    def __init__(self, primary, inweight, idscas, maps, n2, postage_pad, fk):
        if primary.dtype != torch.float32 or primary.dim() != 4 or primary.shape[-1] != primary.shape[-2]:
            raise ValueError(f"ShareBlock: PRIMARY must be float32 [n_out, nlayer, NsideP, NsideP], not {primary.dtype} {tuple(primary.shape)} "
                             "(float64 and I24-compressed layers: convert or decompress them first)")
        if primary.stride(-1) != 1 or primary.stride(0) != primary.shape[1] * primary.stride(1):
            raise ValueError("ShareBlock: PRIMARY needs unit column stride and evenly spaced planes")
        if inweight.dtype != torch.float32 or inweight.dim() != 4 or inweight.shape[-1] != inweight.shape[-2] or not inweight.is_contiguous():
            raise ValueError("ShareBlock: INWEIGHT must be contiguous float32 [n_out, n_inimage, n1P, n1P]")
        idscas = [(int(o), int(s)) for o, s in idscas]
        if len(idscas) != inweight.shape[1] or inweight.shape[0] != primary.shape[0]:
            raise ValueError("ShareBlock: INDATA, INWEIGHT and PRIMARY disagree on n_inimage or n_out")
        for name, (codes, unit, comment) in maps.items():
            if codes.dtype not in (torch.int16, torch.uint16) or tuple(codes.shape) != (primary.shape[0],) + tuple(primary.shape[2:]) or not codes.is_contiguous():
                raise ValueError(f"ShareBlock: {name} must be contiguous (u)int16 [n_out, NsideP, NsideP]")
            int(comment.partition("*")[0])  # (what analysis.py:530 parses)
        self.primary, self.inweight, self.idscas, self.maps = primary, inweight, idscas, dict(maps)
        self.n2, self.postage_pad, self.fk = int(n2), int(postage_pad), int(fk)
        if primary.shape[-1] != inweight.shape[-1] * self.n2:
            raise ValueError(f"ShareBlock: NsideP = {primary.shape[-1]} is not n1P * n2 = {inweight.shape[-1]} * {self.n2}")

    @classmethod
    def from_arrays(cls, primary, inweight, idscas, maps, n2, postage_pad, fk, device="cuda:0"):
        """From host arrays as a FITS reader delivers them: big-endian data is converted to the machine's order; float64 PRIMARY is refused."""
        def native(a):
            a = np.asarray(a)
            return np.ascontiguousarray(a.astype(a.dtype.newbyteorder("="), copy=False))

        primary = native(primary)
        if primary.dtype != np.float32:
            raise ValueError(f"ShareBlock: PRIMARY is {primary.dtype}; only float32 layers are shared (float64 and I24-compressed layers: "
                             "convert or decompress them first)")
        up = lambda a: torch.from_numpy(native(a).copy()).to(device)  # noqa: E731
        return cls(up(primary), up(np.asarray(inweight, dtype=np.float32)), idscas, {k: (up(v[0]), v[1], v[2]) for k, v in maps.items()}, n2, postage_pad, fk)

    @classmethod
    def from_block_maps(cls, bm, fk, idscas, outmaps="USKTN", *, postage_pad):
        """After ``BlockMaps.finalize``: ``primary`` is the view of ``bm.out_map`` cropped by fk (shared, not copied: the update shows in
        ``bm.out_map``), the codes are ``bm.compress(name, fk)`` with the units of coadd.py:2247-2305."""
        if fk != bm.fade:
            raise ValueError(f"from_block_maps: fk = {fk} but the block was coadded with fade = {bm.fade}")
        primary = bm.out_map[:, :, fk:bm.nside - fk, fk:bm.nside - fk]
        maps = {hdu: (bm.compress(name, fk), unit, comment) for hdu, (letter, name, unit, comment) in MAP_HDUS.items() if letter in outmaps}
        return cls(primary, bm.T_weightmap, idscas, maps, bm.n2, postage_pad, fk)

    def inwtflat(self):
        """analysis.py:490-493: INWTFLAT [n_out * n1P, n_inimage * n1P] of the current INWEIGHT."""
        n_out, n_in, n1P = self.inweight.shape[:3]
        return self.inweight.permute(0, 2, 1, 3).reshape(n_out * n1P, n_in * n1P)

    def to_arrays(self):
        """The host arrays for whoever writes the file: dict(primary, inweight, inwtflat, idscas, maps: name -> (codes, unit, comment))."""
        return {"primary": self.primary.cpu().numpy(), "inweight": self.inweight.cpu().numpy(), "inwtflat": self.inwtflat().cpu().numpy(),
                "idscas": list(self.idscas), "maps": {k: (v[0].cpu().numpy(), v[1], v[2]) for k, v in self.maps.items()}}


def update(mine, theirs, direction, add_mode=True, zero_floor=None, ctx=None, sums=None):
    """``mine._update_hdu_data(theirs, direction, add_mode)`` (analysis.py:394-537): PRIMARY, INWEIGHT and every quality map of ``mine`` are
    updated on the side ``direction`` from ``theirs``, which does not change; ``n2``, ``postage_pad`` and ``fk`` are the blocks'.  Whether
    ``pad_sides`` is "auto" is the caller's business.  ``zero_floor``: see ``floor_code``.  ``sums``: None, or a dict that receives name ->
    the float32 strip ``mine * add_mode + theirs`` before the encode (for tests; production passes none)."""
    if direction not in DIRECTIONS:
        raise ValueError(f"direction '{direction}' not supported by update")
    if mine is theirs:
        raise ValueError("a block does not share padding stamps with itself")
    n_out, nlayer, NsideP = mine.primary.shape[0], mine.primary.shape[1], mine.primary.shape[-1]
    n1P = mine.inweight.shape[-1]
    if tuple(theirs.primary.shape) != tuple(mine.primary.shape) or theirs.inweight.shape[-1] != n1P or theirs.inweight.shape[0] != n_out:
        raise ValueError(f"the blocks differ in shape: {tuple(mine.primary.shape)} / {tuple(theirs.primary.shape)}, n1P {n1P} / {theirs.inweight.shape[-1]}")
    if list(mine.maps) != list(theirs.maps) or any(mine.maps[k][0].dtype != theirs.maps[k][0].dtype for k in mine.maps):
        raise ValueError(f"the blocks differ in their maps: {list(mine.maps)} / {list(theirs.maps)}")
    n2, postage_pad, fk = mine.n2, mine.postage_pad, mine.fk
    if (theirs.n2, theirs.postage_pad, theirs.fk) != (n2, postage_pad, fk):
        raise ValueError("the blocks differ in n2, postage_pad or fade_kernel")
    ctx = bound_context(ctx=ctx)
    h, d, add, width = ctx.handle, DIRECTIONS.index(direction), 1 if add_mode else 0, postage_pad * n2
    pm, pu = mine.primary, theirs.primary
    check(lib.imcom_padshare_layers(h, d, add, NsideP, width, fk, n_out * nlayer, ptr(pm), pm.stride(2), pm.stride(1), ptr(pu), pu.stride(2), pu.stride(1)))
    pairs = idsca_pairs(mine.idscas, theirs.idscas)
    check(lib.imcom_padshare_weights(h, d, n_out, n1P, postage_pad, len(pairs), ptr(pairs), ptr(mine.inweight), mine.inweight.shape[1], ptr(theirs.inweight),
                                     theirs.inweight.shape[1]))
    table = (PadshareMap * max(len(mine.maps), 1))()
    along_x = direction in ("left", "right")
    for row, (name, (codes, unit, comment)) in zip(table, mine.maps.items()):
        unsigned = codes.dtype == torch.uint16
        floor = floor_code(unit, comment, unsigned, zero_floor)
        row.mine, row.theirs = codes.data_ptr(), theirs.maps[name][0].data_ptr()
        row.decode_coef = decode_coefficient(unit, comment)
        row.floor_code = PADSHARE_NO_FLOOR if floor is None else floor
        row.encode_coef, row.is_unsigned = int(comment.partition("*")[0]), int(unsigned)
        if sums is not None:
            sums[name] = torch.empty((n_out, NsideP, width + fk) if along_x else (n_out, width + fk, NsideP), dtype=torch.float32, device=codes.device)
            row.sums = sums[name].data_ptr()
    check(lib.imcom_padshare_maps(h, d, add, NsideP, width, fk, n_out, len(mine.maps), C.cast(table, C.c_void_p)))


def share_padding_stamps(nblock, load, save=None, zero_floor=None, ctx=None):
    """``Mosaic.share_padding_stamps`` (analysis.py:1429-1467) in the reference's order: row by row ``right`` adding then ``left`` replacing,
    then column by column ``top`` adding then ``bottom`` replacing.  ``load(iby, ibx)`` returns a ShareBlock, resident or read on demand, and
    ``save(iby, ibx, block)`` is called where the reference saves; no more than two blocks are held at once.  ``load`` may also be a grid
    ``blocks[iby][ibx]`` of resident ShareBlocks, which are then updated in place."""
    if not callable(load):
        grid = load
        load = lambda iby, ibx: grid[iby][ibx]  # noqa: E731
    save = save or (lambda iby, ibx, block: None)
    kw = dict(zero_floor=zero_floor, ctx=ctx)
    for horizontal in (True, False):
        for i in range(nblock):
            at = (lambda j: (i, j)) if horizontal else (lambda j: (j, i))
            low = load(*at(0))
            for j in range(nblock - 1):
                high = load(*at(j + 1))
                update(low, high, "right" if horizontal else "top", add_mode=True, **kw)
                update(high, low, "left" if horizontal else "bottom", add_mode=False, **kw)
                save(*at(j), low)
                low = high
            save(*at(nblock - 1), low)
