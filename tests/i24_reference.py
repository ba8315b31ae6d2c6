"""The I24 codec restated in numpy from its arithmetic (ALPHA = 1), independent of the reference's own text: explicit index maps for the
REORDER bit stream instead of unpackbits / transpose / packbits, a wrapping uint32 cumulative sum, float32 steps one at a time.
tests/test_i24_host.py pins it to the fixtures of the reference (tests/golden/i24.npz) with ==; the device tests then use it for inputs
beyond the fixtures."""

import numpy as np

SCHEMES = ("I24A", "I24B")


def parse(pars):
    """(vmin, vmax, softbias, diff, alpha, bitkeep, reorder) as the reference's constructor reads them."""
    bitkeep = int(pars["BITKEEP"]) if "BITKEEP" in pars else 24
    if "BITKEEP" in pars and (bitkeep >= 24 or bitkeep <= 0):
        raise ValueError(f"Can't keep {bitkeep:d} bits")
    return (float(pars["VMIN"]), float(pars["VMAX"]), int(pars["SOFTBIAS"]) if "SOFTBIAS" in pars else 0, bool(pars["DIFF"]) if "DIFF" in pars else False,
            float(pars["ALPHA"]) if "ALPHA" in pars else 1.0, bitkeep, bool(pars["REORDER"]) if "REORDER" in pars else True)


def stream_fwd(plane):
    """One byte plane [ny, nx] -> the bytes of its bit stream: output byte k, bit t is stream bit s = 8 k + t = bit s // n of pixel s % n."""
    flat = plane.reshape(-1)
    n = flat.size
    out = np.zeros(n, dtype=np.uint8)
    k = np.arange(n, dtype=np.uint32 if 8 * n < 2**32 else np.int64)
    for t in range(8):
        s = 8 * k + t
        out |= (((flat[s % n] >> (s // n).astype(np.uint8)) & 1) << t).astype(np.uint8)
    return out.reshape(plane.shape)


def stream_rev(plane):
    """Inverse: bit b of pixel p is stream bit b n + p."""
    flat = plane.reshape(-1)
    n = flat.size
    out = np.zeros(n, dtype=np.uint8)
    p = np.arange(n, dtype=np.uint32 if 8 * n < 2**32 else np.int64)
    for b in range(8):
        s = b * n + p
        out |= (((flat[s >> 3] >> (s & 7).astype(np.uint8)) & 1) << b).astype(np.uint8)
    return out.reshape(plane.shape)


def quantise(d, vmin, vmax, bitkeep):
    f32 = np.float32
    with np.errstate(all="ignore"):
        c = np.minimum(np.maximum(d, f32(vmin)), f32(vmax))
        y = (c - f32(vmin)) / f32(vmax - vmin)
        f = np.floor(f32(2**bitkeep) * y)
        q = np.where(f > 0, np.minimum(f, f32(2**bitkeep - 1)), f32(0))  # (NaN: 0)
    return q.astype(np.int32)


def ints_fwd(q, B, softbias, diff):
    """DIFF, then SOFTBIAS, of an int32 image of codes."""
    shape, M = q.shape, 2**B
    q = q.reshape(-1).astype(np.int64)
    if diff:
        q[1:] = (q[1:] - q[:-1]) % M
    if softbias > 0:
        q = (softbias + q) % M
    elif softbias == -1:
        q = np.where(q >= M // 2, 2 * (M - q) - 1, 2 * q)
    return q.astype(np.int32).reshape(shape)


def ints_rev(q, B, softbias, diff):
    """SOFTBIAS back, then DIFF back (a wrapping uint32 prefix sum over the flat image, masked), in int32 as numpy has it."""
    shape, M = q.shape, 2**B
    with np.errstate(over="ignore"):
        if softbias > 0:
            q = ((np.int32(M - softbias) + q) & np.int32(M - 1)).astype(np.int32)
        elif softbias == -1:
            q = np.where(q & 1, np.int32(M - 1) - (q >> 1), q >> 1).astype(np.int32)
        if diff:
            q = (np.cumsum(np.ascontiguousarray(q).reshape(-1).view(np.uint32), dtype=np.uint32) & np.uint32(M - 1)).astype(np.int32).reshape(shape)
    return q


def compress(im, scheme, pars):
    """(data, (y, x, value)) of a float32 image."""
    vmin, vmax, softbias, diff, alpha, B, reorder = parse(pars)
    assert alpha == 1.0 and scheme in SCHEMES and im.dtype == np.float32 and im.ndim == 2
    ny, nx = im.shape
    with np.errstate(invalid="ignore"):
        hit = np.flatnonzero((im.reshape(-1) < np.float32(vmin)) | (im.reshape(-1) > np.float32(vmax)))
    table = ((hit // nx).astype(np.int32), (hit % nx).astype(np.int32), im.reshape(-1)[hit].copy())
    q = ints_fwd(quantise(im, vmin, vmax, B), B, softbias, diff)
    if scheme == "I24A":
        return q, table
    nb = (B + 7) // 8
    cube = np.stack([((q >> (8 * j)) & 255).astype(np.uint8) for j in range(nb)])
    if reorder:
        cube = np.stack([stream_fwd(cube[j]) for j in range(nb)])
    return cube, table


def decompress(im, scheme, pars, overflow=None):
    """float32 image of an int32 image (I24A) or a uint8 cube (I24B); overflow: (y, x, value) or None."""
    vmin, vmax, softbias, diff, alpha, B, reorder = parse(pars)
    assert alpha == 1.0 and scheme in SCHEMES
    M = 2**B
    if im.dtype == np.uint8:
        planes = [stream_rev(im[j]) if reorder else im[j] for j in range(im.shape[0])]
        q = np.zeros(im.shape[1:], dtype=np.int32)
        for j, pl in enumerate(planes):
            q += pl.astype(np.int32) << (8 * j)
    else:
        q = im.astype(np.int32)
    q = ints_rev(q, B, softbias, diff)
    y = (0.5 + q.astype(np.float64)) / float(M)
    prod = (vmax - vmin) * y
    out = (vmin + prod).astype(np.float32)
    if overflow is not None:
        oy, ox, ov = (np.asarray(a) for a in overflow)
        out[oy, ox] = ov
    return out
