"""numpy's normal draws on the device, and the white-noise layer made of them (reference src/pyimcom/layer.py:1297-1305).

The reference regenerates ``whitenoise<q>`` for every input image of every block: ``default_rng(seed).normal(size=(4088, 4088))``.
``Generator.standard_normal`` is a ziggurat over the PCG64 stream: 99.3 % of the draws take one 64-bit output, the others take more, so a
draw has no stream position of its own.  csrc/ziggurat.hip finds the draws as a chain through the stream (every position has an "attempt
starting here"; the draws are the emitting attempts on the chain) by pointer doubling inside tiles and a walk over the tiles, with the
tables of the installed numpy (csrc/ziggurat_tables.h).  Every draw equals numpy's bit for bit:

* the two comparisons of the draw that depend on ``exp`` / ``log1p`` are made with a guard band; a call with a comparison inside the band
  is *undecided* and the request is drawn by numpy on the host instead (``info["undecided"]``; about one call in 7 10^5 at 4088^2 draws);
* the tail draws (|x| > 3.654, 2.7e-4 of all) hold ``log1p``'s last bit: the device returns where they go and the words they are made of,
  and they are formed here with ``math.log1p``, the libm function numpy calls, and patched in with one scatter.

The binding (seam 13): the two lines layer.py:1303-1304 become

    inimage.indata[i, :, :] = pyimcom_amd.noiselayers.white_noise_frame(seed, Stn.sca_nside)

and ``CplxNoise.noise_1f_frame`` (layer.py:871-913) is bound as a whole:

    pyimcom.layer.CplxNoise.noise_1f_frame = staticmethod(pyimcom_amd.noiselayers.noise_1f_frame)

Its 2 x 32 x 2^20 draws are made as above and stay on the device; csrc/noise1f.hip transforms them (a float64 four-step DFT per channel),
subtracts the channel means, casts to float32 and lays the channels into the frame.  The draws are numpy's bit for bit; the transform is
another float64 evaluation of the same sums than pocketfft's, so a pixel can differ from the reference's by one float32 unit in the last
place where the two float64 values lie on either side of a float32 rounding boundary (tests/test_gpu_noise1f.py bounds how often).

``Generator.poisson(lam=array)``, the noise of the ``nstar`` layer (layer.py:1385-1387), is served too (``poisson``; INTEGRATION.md, seam
22): a Poisson draw consumes a number of outputs that depends on its rate and on the outputs, so the draws are a path through (draw,
position) that csrc/poisson.hip finds superchunk by superchunk through windows of candidate positions.  Its comparisons that depend on
``log`` / ``exp`` carry a guard band as well (csrc/poisson_core.h); an undecided request, at most one 4088^2 frame in 1.2e4, is drawn by numpy."""

import ctypes as C
import math

import numpy as np

from ._dev import bound_context, out_array
from ._lib import MEM_DEVICE, check, lib, ptr
from .simmask import halves

__all__ = ["standard_normal", "normal", "white_noise_frame", "noise_1f", "noise_1f_amp", "noise_1f_frame", "poisson", "last_info", "last_poisson_info"]

ZIG_R = 3.6541528853610088  # numpy/random/src/distributions/ziggurat_constants.h: ziggurat_nor_r, ziggurat_nor_inv_r
ZIG_INV_R = 0.27366123732975828
last_info = {}  # the info of the last call of standard_normal
last_poisson_info = {}  # the info of the last call of poisson / of inject.nstar_layer


def _bitgen(bitgen_or_seed):
    """(the PCG64 to leave advanced or None, state, inc)."""
    if isinstance(bitgen_or_seed, np.random.Generator):
        bitgen_or_seed = bitgen_or_seed.bit_generator
    if isinstance(bitgen_or_seed, np.random.BitGenerator):
        if not isinstance(bitgen_or_seed, np.random.PCG64):
            raise TypeError(f"only np.random.PCG64 streams are served, not {type(bitgen_or_seed).__name__}")
        bg, keep = bitgen_or_seed, bitgen_or_seed
    elif isinstance(bitgen_or_seed, (int, np.integer, np.random.SeedSequence)):
        bg, keep = np.random.PCG64(bitgen_or_seed), None
    else:
        raise TypeError(f"a seed or an np.random.PCG64 is expected, not {type(bitgen_or_seed).__name__}")
    st = bg.state["state"]
    return keep, bg, int(st["state"]), int(st["inc"])


def tail_values(raw):
    """The tail draws of numpy from their two stream outputs (uint64 [n, 2]): +-(r - log1p(-u) / r) with libm's log1p."""
    vals = np.empty(len(raw))
    for j, (w0, w1) in enumerate(raw.tolist()):
        xx = -ZIG_INV_R * math.log1p(-((w1 >> 11) * 2.0**-53))
        vals[j] = -(ZIG_R + xx) if (w0 >> 17) & 1 else ZIG_R + xx
    return vals


def standard_normal(bitgen_or_seed, shape, offset=0, device=None, return_info=False, _guard=0.0, _tile=0, _chunk_tiles=0):
    """What ``Generator(bg).standard_normal(shape)`` returns after ``bg.advance(offset)``: float64, a numpy array or with ``device`` a torch
    tensor there.  A ``np.random.PCG64`` (or a Generator of one) passed in is left advanced by ``offset`` and the outputs the draws
    consumed, as numpy leaves it; any other bit generator raises TypeError.  ``return_info``: also a dict with the outputs ``consumed``,
    the ``slow`` attempts, the ``tails`` patched and ``undecided`` (1: the draws came from numpy on the host).  The arguments with an
    underscore are for tests: the guard band, the tile size and the tiles of a chunk; no result depends on them."""
    keep, bg, state, inc = _bitgen(bitgen_or_seed)
    offset, _tile, _chunk_tiles, _guard = int(offset), int(_tile), int(_chunk_tiles), float(_guard)
    if (_tile and (_tile < 4 or _tile > 1024 or _tile & (_tile - 1))) or not 0 <= _chunk_tiles <= 1 << 20 or not 0.0 <= _guard <= 1.0:
        raise ValueError("standard_normal: _tile is a power of two in 4 .. 1024, _chunk_tiles at most 2^20, _guard in 0 .. 1")
    shape = (int(shape),) if np.ndim(shape) == 0 else tuple(int(s) for s in shape)
    if offset < 0 or offset >= 1 << 128 or any(s < 0 for s in shape):
        raise ValueError("standard_normal: offset in 0 .. 2^128 - 1 and a shape without negative sides")
    count = int(np.prod(shape, dtype=object)) if shape else 1
    out, mem, ctx = out_array(shape, np.float64, device)
    cap = C.c_long(0)
    check(lib.imcom_pcg64_normal_sizes(count, C.byref(cap)))
    tail_idx, _, _ = out_array((cap.value,), np.int64, device)
    tail_raw, _, _ = out_array((cap.value, 2), np.uint64 if device is None else np.int64, device)
    info = np.zeros(4, dtype=np.uint64)
    check(lib.imcom_pcg64_normal_ex(ctx.handle, *halves(state), *halves(inc), *halves(offset), count, ptr(out) if count else None,
                                    ptr(tail_idx) if count else None, ptr(tail_raw) if count else None, ptr(info), mem, _tile, _chunk_tiles, _guard))
    consumed, slow, tails, undecided = (int(v) for v in info)
    if undecided:  # the whole request from numpy; the state it leaves is the one to keep
        host = np.random.PCG64()
        host.state = bg.state
        if offset:
            host.advance(offset)
        draws = np.random.Generator(host).standard_normal(shape)
        if device is None:
            out = draws
        else:
            import torch

            out.copy_(torch.from_numpy(np.ascontiguousarray(draws)))
        if keep is not None:
            keep.state = host.state
        consumed = None
    else:
        if tails:
            if device is None:
                order = np.argsort(tail_idx[:tails], kind="stable")
                out.reshape(-1)[tail_idx[:tails][order]] = tail_values(tail_raw[:tails][order])
            else:
                import torch

                idx = tail_idx[:tails].cpu().numpy()
                order = np.argsort(idx, kind="stable")
                vals = tail_values(tail_raw[:tails].cpu().numpy().view(np.uint64)[order])
                out.view(-1).index_put_((torch.from_numpy(idx[order]).to(out.device),), torch.from_numpy(vals).to(out.device))
        if keep is not None and offset + consumed:
            st = keep.state  # advance() drops the cached half of a 64-bit output (has_uint32 / uinteger); standard_normal leaves it
            keep.advance((offset + consumed) % (1 << 128))
            after = keep.state
            after["has_uint32"], after["uinteger"] = st["has_uint32"], st["uinteger"]
            keep.state = after
    last_info.clear()
    last_info.update(consumed=consumed, slow=slow, tails=tails, undecided=undecided)
    return (out, dict(last_info)) if return_info else out


def normal(rng, loc=0.0, scale=1.0, size=None, device=None):
    """``rng.normal(loc, scale, size)`` for scalar ``loc`` and ``scale``: ``loc + scale * x`` of the standard draws x, as numpy forms it.
    ``rng`` (a Generator of a PCG64, or the PCG64) is left advanced; ``size`` None gives a float."""
    loc, scale = float(loc), float(scale)
    if scale < 0 or math.isnan(scale):
        raise ValueError("scale < 0")
    x = standard_normal(rng, () if size is None else size, device=device)
    x = loc + scale * x
    return float(x) if size is None else x


def white_noise_frame(seed, nside, device=None):
    """The right-hand side of layer.py:1303-1304: ``default_rng(seed).normal(loc=0.0, scale=1.0, size=(nside, nside))``, float64."""
    return normal(np.random.PCG64(int(seed)), 0.0, 1.0, (int(nside), int(nside)), device=device)


def noise_1f_amp(length):
    """The amplitudes of layer.py:892-895, formed in numpy exactly as there: |frequency index|^-1/2, zero at frequency zero."""
    freq = np.linspace(0, 1 - 1.0 / length, length)
    freq[length // 2 :] -= 1.0
    amp = (1.0e-99 + np.abs(freq * length)) ** (-0.5)
    amp[0] = 0.0
    return amp


def noise_1f(normals, amp, nch, w, border=4, return_block=False):
    """The channel loop of layer.py:896-913 and the crop of 913 on the device, for ``normals`` [2 nch, len] (a float64 tensor on the device:
    rows 2c, 2c + 1 are the real and imaginary draws of channel c) and ``amp`` [len] (numpy): the float32 frame [len / 2 / w - 2 border,
    nch w - 2 border] as a tensor there; ``return_block``: also the float64 channels [nch, len / 2] before the cast.  The reference has
    len = 2^20, nch = 32, w = 128; len and w are powers of two, len in 2^10 .. 2^20 (else ImcomError, status unsupported)."""
    import torch

    nch, w, border = int(nch), int(w), int(border)
    if not (isinstance(normals, torch.Tensor) and normals.is_cuda and normals.dtype == torch.float64 and normals.dim() == 2 and normals.shape[0] == 2 * nch):
        raise ValueError("noise_1f: normals is a float64 tensor [2 nch, len] on the device")
    normals = normals.contiguous()
    length = int(normals.shape[1])
    amp = np.ascontiguousarray(amp, dtype=np.float64)
    if amp.shape != (length,):
        raise ValueError("noise_1f: amp has one entry per draw of a channel")
    dev = normals.device
    ctx = bound_context(dev)
    shape = (max(length // 2 // max(w, 1) - 2 * border, 0), max(nch * w - 2 * border, 0))
    frame = torch.empty(shape, dtype=torch.float32, device=dev)
    block = torch.empty((nch, length // 2), dtype=torch.float64, device=dev) if return_block else None
    amp_d = torch.from_numpy(amp).to(dev)
    check(lib.imcom_noise_1f(ctx.handle, ptr(normals), ptr(amp_d), length, nch, w, border, ptr(frame), ptr(block), MEM_DEVICE))
    return (frame, block) if return_block else frame


def noise_1f_frame(seed, device_out=False, _length=8192 * 128, _nch=32, _w=128):
    """``CplxNoise.noise_1f_frame(seed)`` (layer.py:871-913): the float32 [4088, 4088] frame of 1/f noise, independent in each of the 32
    channels; a numpy array, or with ``device_out`` the tensor on the device.  The arguments with an underscore are for tests."""
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    normals = standard_normal(np.random.PCG64(int(seed)), (2 * _nch, _length), device=dev)
    frame = noise_1f(normals, noise_1f_amp(_length), _nch, _w)
    return frame if device_out else frame.cpu().numpy()


def _leave_advanced(keep, steps):
    """``keep`` (a PCG64) ``steps`` outputs on, with its cached 32-bit half as it was (advance() drops it; the draws leave it)."""
    if keep is None or not steps:
        return
    st = keep.state
    keep.advance(steps % (1 << 128))
    after = keep.state
    after["has_uint32"], after["uinteger"] = st["has_uint32"], st["uinteger"]
    keep.state = after


def _host_generator(bg, offset):
    host = np.random.PCG64()
    host.state = bg.state
    if offset:
        host.advance(offset)
    return host


def _poisson_call(bitgen_or_seed, offset, values, shape, out_dtype, device, call, host_draw, who):
    """The frame of ``poisson`` and ``inject.nstar_layer``: the output array, the library call ``call(ctx, stream halves, pointers)``, the
    request drawn by numpy (``host_draw(Generator)``) when the device is undecided or a rate is invalid (numpy raises its ValueError), and
    the state a PCG64 passed in is left in.  ``values``: the rates or the brightness, numpy or a tensor on the device."""
    from ._dev import is_torch, staged

    keep, bg, state, inc = _bitgen(bitgen_or_seed)
    offset = int(offset)
    if offset < 0 or offset >= 1 << 128:
        raise ValueError(f"{who}: offset in 0 .. 2^128 - 1")
    if is_torch(values) and values.is_cuda and device is None:
        device = values.device
    out, mem, ctx = out_array(shape, out_dtype, device)
    if device is not None:
        values = staged(values, out.device, astype=np.float64)
    count = int(np.prod(shape, dtype=object)) if shape else 1
    info = np.zeros(4, dtype=np.uint64)
    rc = call(ctx, halves(state) + halves(inc) + halves(offset), ptr(values) if count else None, count, ptr(out) if count else None, ptr(info), mem)
    consumed, undecided, recovered, invalid = (int(v) for v in info)
    if not invalid:
        check(rc)
    if undecided or invalid:  # the whole request from numpy (which raises for an invalid rate); the state it leaves is the one to keep
        host = _host_generator(bg, offset)
        draws = host_draw(np.random.Generator(host), values.cpu().numpy() if is_torch(values) else values)
        if device is None:
            out = draws
        else:
            import torch

            out.copy_(torch.from_numpy(np.ascontiguousarray(draws)))
        if keep is not None:
            keep.state = host.state
        consumed = None
    else:
        _leave_advanced(keep, offset + consumed)
    last_poisson_info.clear()
    last_poisson_info.update(consumed=consumed, undecided=undecided, recovered=recovered)
    return out, dict(last_poisson_info)


def poisson(bitgen_or_seed, lam, offset=0, device=None, return_info=False, _superchunk=0, _window=0, _tile=0, _guard=None, _force_walk=False):
    """What ``Generator(bg).poisson(lam=lam)`` returns after ``bg.advance(offset)``: int64 of ``lam``'s shape, bit for bit; a numpy array, or a
    torch tensor on the device when ``lam`` is one there or ``device`` is given.  A ``np.random.PCG64`` (or a Generator of one) passed in
    is left advanced by ``offset`` and the outputs the draws consumed, as numpy leaves it; any other bit generator raises TypeError.  A
    rate that is negative, NaN or too large raises numpy's ValueError.  ``return_info``: also a dict with the outputs ``consumed``,
    ``undecided`` (1: the draws came from numpy on the host) and the superchunks ``recovered`` by the sequential walk.  The arguments with
    an underscore are for tests: the draws of a superchunk, the window, the draws of a tile, the guard band (None: the production band,
    0: none, 1: everything undecided) and the walk for every superchunk; no result depends on them."""
    from ._dev import is_torch

    if is_torch(lam) and not lam.is_cuda:
        lam = lam.numpy()
    if not is_torch(lam):
        lam = np.ascontiguousarray(lam, dtype=np.float64)
    shape = tuple(int(s) for s in lam.shape)
    guard = -1.0 if _guard is None else float(_guard)
    if not 0 <= int(_superchunk) <= 65536 or not 0 <= int(_window) <= 4096 or not 0 <= int(_tile) <= 4096 or guard > 1.0:
        raise ValueError("poisson: _superchunk at most 65536, _window and _tile at most 4096, _guard at most 1")

    def call(ctx, stream, values, count, out, info, mem):
        return lib.imcom_pcg64_poisson_ex(ctx.handle, *stream, values, count, out, info, mem, int(_superchunk), int(_window), int(_tile), guard,
                                          int(bool(_force_walk)))

    out, info = _poisson_call(bitgen_or_seed, offset, lam, shape, np.int64, device, call, lambda g, v: g.poisson(lam=v.reshape(shape)), "poisson")
    return (out, info) if return_info else out
