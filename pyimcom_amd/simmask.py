"""Simulated cosmic-ray masks and sub-sampled uniform draws on the device: ``Mask.randmask`` and ``Mask.load_cr_mask`` (reference
src/pyimcom/layer.py:933-964, 1049-1082), ``GalSimInject.subgen`` / ``subgen_multirow`` (layer.py:313-401).

The reference draws ``default_rng(100000000 + obsid).uniform(size=(18, 4108, 4108))`` -- 3.04e8 doubles, 2.4 GB -- for every input image
of every block and keeps one slice of it.  numpy's default generator is PCG64, a 128-bit LCG with an output permutation: draw k of the
stream is a closed form of (state, increment, k).  csrc/pcg64.hip forms every draw where it is needed, in integer arithmetic, equal to
numpy's bit for bit; the mask kernel keeps its hits in LDS and writes the uint8 mask alone.  The binding (seam 10):

    pyimcom.layer.Mask.randmask = staticmethod(pyimcom_amd.simmask.randmask)
    pyimcom.layer.GalSimInject.subgen = staticmethod(pyimcom_amd.simmask.subgen)

Seeding stays numpy's, on the host: the state and increment are read from ``np.random.PCG64(seed).state``.  Only draws that take one
64-bit output each are served here (``uniform`` / ``random``): numpy's normal and Poisson draws (the white-noise and 1/f layers,
layer.py:1297-1313; the ``nstar`` layer) consume a data-dependent number of outputs and are served by ``pyimcom_amd.noiselayers``.

Outputs are numpy arrays (host memspace) or torch CUDA tensors (device memspace, on torch's current stream)."""

import numpy as np

from ._dev import compare_value, is_torch, out_array
from ._lib import check, lib, ptr

__all__ = ["uniform", "uniform_at", "cr_mask", "randmask", "load_cr_mask", "subgen", "subgen_multirow"]

PAD = 10  # layer.py:956
N_SLICES = 18  # layer.py:957: one slice per SCA
SEED0 = 100000000  # layer.py:954
_M64 = (1 << 64) - 1


def _stream(bitgen_or_seed):
    """(state, inc) of a PCG64 stream: of the given ``np.random.PCG64`` as it stands (it is not advanced), or of ``PCG64(seed)``."""
    if isinstance(bitgen_or_seed, np.random.Generator):
        bitgen_or_seed = bitgen_or_seed.bit_generator
    if isinstance(bitgen_or_seed, np.random.BitGenerator):
        if not isinstance(bitgen_or_seed, np.random.PCG64):
            raise TypeError(f"only np.random.PCG64 streams are served, not {type(bitgen_or_seed).__name__}")
        bg = bitgen_or_seed
    elif isinstance(bitgen_or_seed, (int, np.integer)) or isinstance(bitgen_or_seed, np.random.SeedSequence):
        bg = np.random.PCG64(bitgen_or_seed)
    else:
        raise TypeError(f"a seed or an np.random.PCG64 is expected, not {type(bitgen_or_seed).__name__}")
    st = bg.state["state"]
    return int(st["state"]), int(st["inc"])


def halves(v):
    return v & _M64, (v >> 64) & _M64


def uniform(bitgen_or_seed, offset, shape, device=None):
    """Draws ``offset`` .. ``offset + prod(shape) - 1`` of the stream, in C order: what ``Generator(bg).uniform(size=shape)`` returns after
    ``bg.advance(offset)``.  float64; numpy, or a tensor on ``device``.  A given bit generator is left as it is."""
    state, inc = _stream(bitgen_or_seed)
    offset = int(offset)
    shape = (int(shape),) if np.ndim(shape) == 0 else tuple(int(s) for s in shape)
    if offset < 0 or offset >= 1 << 128 or any(s < 0 for s in shape):
        raise ValueError("uniform: offset in 0 .. 2^128 - 1 and a shape without negative sides")
    count = int(np.prod(shape, dtype=object)) if shape else 1
    out, mem, ctx = out_array(shape, np.float64, device)
    check(lib.imcom_pcg64_uniform(ctx.handle, *halves(state), *halves(inc), *halves(offset), count, ptr(out) if count else None, mem))
    return out


def uniform_at(bitgen_or_seed, positions, device=None):
    """Draws ``positions`` (integers >= 0 of any shape, in any order) of the stream, float64 of the same shape.  ``positions`` may be a
    torch tensor on ``device``."""
    state, inc = _stream(bitgen_or_seed)
    if is_torch(positions):
        import torch

        if device is None:
            device = positions.device
        pos = positions.to(device=device, dtype=torch.int64).contiguous()
        neg = bool((pos < 0).any().item()) if pos.numel() else False
    else:
        pos = np.asarray(positions)
        if pos.size and not np.issubdtype(pos.dtype, np.integer):
            raise TypeError("uniform_at: integer positions")
        if pos.size and int(pos.max()) >= 1 << 63:
            raise ValueError("uniform_at: positions below 2^63")
        pos = np.ascontiguousarray(pos, dtype=np.int64)
        neg = bool((pos < 0).any())
        if device is not None:
            import torch

            pos = torch.as_tensor(pos, device=device)
    if neg:
        raise ValueError("uniform_at: positions are not negative")
    out, mem, ctx = out_array(tuple(pos.shape), np.float64, device)
    count = int(np.prod(tuple(pos.shape), dtype=object))
    check(lib.imcom_pcg64_uniform_at(ctx.handle, *halves(state), *halves(inc), ptr(pos) if count else None, count, ptr(out) if count else None, mem))
    return out


def cr_mask(bitgen_or_seed, nside, sca_slice, pcut, labnoise=None, threshold=0.0, pad=PAD, n_slices=N_SLICES, device=None):
    """The kernel of ``randmask``: (mask uint8 [nside, nside], number of good pixels) for slice ``sca_slice`` of the padded draw
    [n_slices, nside + 2 pad, nside + 2 pad] of the stream; with ``labnoise`` (float32 [nside, nside]) also ``|labnoise| < threshold``."""
    state, inc = _stream(bitgen_or_seed)
    nside = int(nside)
    if nside < 1:
        raise ValueError("cr_mask: nside >= 1")
    if labnoise is not None:
        if is_torch(labnoise):
            import torch

            if labnoise.dtype != torch.float32:
                raise TypeError("cr_mask: a float32 labnoise layer")
            labnoise = labnoise.contiguous() if device is None or labnoise.device == torch.device(device) else labnoise.to(device).contiguous()
            if device is None:
                device = labnoise.device
        else:
            labnoise = np.asarray(labnoise)
            if labnoise.dtype != np.float32:
                raise TypeError("cr_mask: a float32 labnoise layer")
            labnoise = np.ascontiguousarray(labnoise)
            if device is not None:
                import torch

                labnoise = torch.as_tensor(labnoise, device=device)
        if tuple(labnoise.shape) != (nside, nside):
            raise ValueError(f"cr_mask: labnoise of shape {tuple(labnoise.shape)} for nside {nside}")
        threshold = compare_value(threshold, np.float32)
    mask, mem, ctx = out_array((nside, nside), np.uint8, device)
    ngood, _, _ = out_array((1,), np.int64, device)
    check(lib.imcom_cr_mask(ctx.handle, *halves(state), *halves(inc), nside, int(pad), int(sca_slice), int(n_slices), float(pcut), ptr(labnoise),
                            float(threshold), ptr(mask), ptr(ngood), mem))
    return mask, int(ngood[0])


def _sca_nside():
    try:
        from pyimcom.config import Settings  # the reference package, when this runs as its plug-in

        return int(Settings.sca_nside)
    except ImportError:
        return 4088  # config.py:98


def randmask(idsca, pcut, hitinfo=None, *, nside=None, device_out=False, device="cuda:0"):
    """``Mask.randmask(idsca, pcut)`` (layer.py:933-964): True for good pixels, False for pixels within one pixel of a simulated hit.
    numpy bool [nside, nside] (``nside``: ``Settings.sca_nside``, 4088 without the reference package); with ``device_out`` the uint8
    tensor on ``device`` that ``select.partition_pixels(mask=...)`` takes as it is.  ``hitinfo`` other than None returns None, as the
    reference does."""
    if hitinfo is not None:
        return None
    nside = _sca_nside() if nside is None else int(nside)
    mask, _ = cr_mask(SEED0 + int(idsca[0]), nside, int(idsca[1]) - 1, pcut, device=device if device_out else None)
    return mask if device_out else mask.view(np.bool_)


def load_cr_mask(inimage):
    """``Mask.load_cr_mask(inimage)`` (layer.py:1049-1082): None unless ``cfg.cr_mask_rate > 0``; the random mask of ``inimage.idsca``,
    and-ed with ``|labnoise| < cfg.labnoisethreshold`` in the same launch when "labnoise" is among ``cfg.extrainput``.  numpy bool."""
    config = inimage.blk.cfg
    if not config.cr_mask_rate > 0:
        return None
    try:
        idx = config.extrainput.index("labnoise")
    except (KeyError, ValueError, AttributeError):
        idx = None
    seed, sl = SEED0 + int(inimage.idsca[0]), int(inimage.idsca[1]) - 1
    if idx is None:
        nside = _sca_nside()
        mask, ngood = cr_mask(seed, nside, sl, config.cr_mask_rate)
        print("Cosmic ray mask: good pix --> ", ngood, "/", 4088**2)
        return mask.view(np.bool_)
    lab = inimage.indata[idx]
    if not is_torch(lab):
        lab = np.asarray(lab)
        if lab.dtype != np.float32:  # (the reference's indata is float32, layer.py:1246-1252; anything else is compared as numpy would)
            raise TypeError(f"load_cr_mask: the labnoise layer is {lab.dtype}, float32 expected")
    nside = int(lab.shape[-1])
    mask, ngood = cr_mask(seed, nside, sl, config.cr_mask_rate, labnoise=lab, threshold=config.labnoisethreshold)
    if is_torch(mask):
        mask = mask.cpu().numpy()
    print("Lab noise threshold: good pix --> ", ngood, "/", 4088**2)
    return mask.view(np.bool_)


def _advance(rngX, delta):
    """``GalSimInject._advance`` (layer.py:286-311) as one call: the reference cuts ``delta`` into steps of 2^30 because it converts the
    remainder through int32; ``PCG64.advance`` takes the whole distance, and the state it leaves is the same."""
    if delta:
        rngX.advance(int(delta) % (1 << 128))


def subgen_multirow(rngX, lenpix, subpix, P, device=None):
    """``GalSimInject.subgen_multirow`` (layer.py:366-401): out[j, i] = R_j[subpix[i]], R_j the j-th run of ``lenpix`` draws of ``rngX``
    from where it stands; ``rngX`` (a ``np.random.PCG64``) is left advanced by ``P * lenpix``."""
    state, inc = _stream(rngX)
    lenpix, P = int(lenpix), int(P)
    sub = np.asarray(subpix).ravel()
    if sub.size and not np.issubdtype(sub.dtype, np.integer):
        sub = sub.astype(np.int64)
    if sub.size == 0 or P <= 0:
        out = np.zeros((max(P, 0), 0))
    elif int(sub.min()) < 0:
        raise ValueError("subgen: entries of subpix are not negative")
    elif (P - 1) * lenpix + int(sub.max()) < 1 << 63:
        out = uniform_at(rngX, np.arange(P, dtype=np.int64)[:, None] * lenpix + sub.astype(np.int64)[None, :], device=device)
    else:  # positions beyond int64: every row from a copy of the stream moved to its start on the host
        rows = []
        for j in range(P):
            bg = np.random.PCG64()
            bg.state = rngX.state
            _advance(bg, j * lenpix)
            rows.append(uniform_at(bg, sub, device=device))
        out = np.stack(rows) if device is None else __import__("torch").stack(rows)
    _advance(rngX, P * lenpix)
    return out


def subgen(rngX, lenpix, subpix, device=None):
    """``GalSimInject.subgen`` (layer.py:313-364): R[subpix] out of the next ``lenpix`` draws R of ``rngX``, in the order of ``subpix``
    (unsorted is fine); ``rngX`` is left advanced by ``lenpix``.  An empty ``subpix`` returns ``np.zeros(0)`` and still advances."""
    if np.size(subpix) == 0:
        _stream(rngX)
        _advance(rngX, int(lenpix))
        return np.zeros(0)
    return subgen_multirow(rngX, lenpix, subpix, 1, device=device)[0]
