"""A numpy restatement of the array statements of ``MetaMosaic`` (reference src/pyimcom/meta/distortimage.py) for the sizes that
tests/golden/metamosaic.npz does not hold, and the synthetic block files both the fixture's generator and the tests use.  It is compared with
the fixture -- the reference's own statements -- in tests/test_metamosaic_host.py.  No device, no astropy."""

import re

import numpy as np

FID_UNIT, SIG_UNIT = "-0.2mB", "0.2mB"


def unit_to_bels(unit, comment=""):
    """helper.py:19-82 (UNIT_to_bels and the legacy sign of HDU_to_bels): a Python float, NaN where the unit does not parse."""
    s = re.match(r"([\d\.\-\+eE]+)([mun]?)B", unit)
    if not s:
        return float("nan")
    x = float(s.group(1))
    x *= {"m": 1e-3, "u": 1e-6, "n": 1e-9}.get(s.group(2), 1.0) if s.group(2) else 1.0
    if x > 0 and comment[:1] == "-":
        x = -x
    return x


def decibels(codes, bels, divisor):
    """197-207: float32, two roundings."""
    return codes.astype(np.float32) * bels / divisor


def axis_windows(n12, padpix, trunc, nside, at_low_edge, at_high_edge, single):
    """The windows of one axis (146-170) in closed form: [(d, smin, smax, c)]."""
    out = []
    for d in ((0,) if single else (-1, 0, 1)):
        c = n12 * (1 + d) - padpix - trunc
        smin = max(0 if at_low_edge else padpix, -c)
        smax = min(padpix + n12 + (padpix if at_high_edge else 0), nside - c)
        out.append((d, smin, smax, c))
    return out


def windows(cfg, ix, iy, bbox=None, extpix=None):
    n12, padpix, nblock = cfg["n1"] * cfg["n2"], cfg["postage_pad"] * cfg["n2"], cfg["nblock"]
    trunc = 0 if extpix is None else max(n12 - extpix, 0)
    nside = 3 * n12 - 2 * trunc
    single = extpix is not None and extpix <= 0
    x0, x1, y0, y1 = (0, nblock, 0, nblock) if bbox is None else bbox
    out = []
    for dx, sxmin, sxmax, cx in axis_windows(n12, padpix, trunc, nside, ix == 0, ix == nblock - 1, single):
        for dy, symin, symax, cy in axis_windows(n12, padpix, trunc, nside, iy == 0, iy == nblock - 1, single):
            if x0 <= ix + dx < x1 and y0 <= iy + dy < y1:
                out.append((dx, dy, ix + dx, iy + dy, symin, symax, sxmin, sxmax, cx, cy))
    return trunc, nside, out


def paste(arrays, window, primary, fid_codes, sig_codes, fid_bels, sig_bels):
    """193-207 for one window = (symin, symax, sxmin, sxmax, cx, cy) into arrays = (in_image, in_fidelity, in_noise)."""
    symin, symax, sxmin, sxmax, cx, cy = window
    dst = (slice(symin + cy, symax + cy), slice(sxmin + cx, sxmax + cx))
    src = (slice(symin, symax), slice(sxmin, sxmax))
    arrays[0][(slice(None),) + dst] = primary[(slice(None),) + src]
    arrays[1][dst] = decibels(fid_codes[src], fid_bels, -0.1)
    arrays[2][dst] = decibels(sig_codes[src], sig_bels, 0.1)


def build(cfg, ix, iy, nlayer, dtype, blocks, bbox=None, extpix=None):
    """The constructor's four arrays (126-210) from blocks[(in_x, in_y)] = dict(primary, fidelity, sigma, fid_bels, sig_bels)."""
    trunc, nside, wins = windows(cfg, ix, iy, bbox, extpix)
    arrays = (np.zeros((nlayer, nside, nside), dtype=dtype), np.zeros((nside, nside), dtype=np.float32), np.zeros((nside, nside), dtype=np.float32))
    for w in wins:
        b = blocks[(w[2], w[3])]
        paste(arrays, w[4:], b["primary"], b["fidelity"], b["sigma"], b["fid_bels"], b["sig_bels"])
    return arrays + (arrays[1] == 0,)


def caps(mask, x, y, r):
    """340-352 on ``mask`` in place."""
    ns = mask.shape[-1]
    for j in range(len(x)):
        xmin = max(int(np.floor(x[j] - r[j])), 0)
        xmax = min(int(np.ceil(x[j] + r[j])) + 1, ns)
        ymin = max(int(np.floor(y[j] - r[j])), 0)
        ymax = min(int(np.ceil(y[j] + r[j])) + 1, ns)
        if xmax <= xmin or ymax <= ymin:
            continue
        erx, ery = np.meshgrid(np.arange(xmin, xmax) - x[j], np.arange(ymin, ymax) - y[j])
        mask[ymin:ymax, xmin:xmax] |= np.hypot(erx, ery) < r[j]
    return mask


def cap_margin(x, y, r, ns):
    """The smallest |d^2 - r^2| / r^2 over the pixels the loop tests (np.longdouble); inf where nothing is tested."""
    L, best = np.longdouble, np.inf
    for j in range(len(x)):
        xmin, xmax = max(int(np.floor(x[j] - r[j])), 0), min(int(np.ceil(x[j] + r[j])) + 1, ns)
        ymin, ymax = max(int(np.floor(y[j] - r[j])), 0), min(int(np.ceil(y[j] + r[j])) + 1, ns)
        if xmax <= xmin or ymax <= ymin:
            continue
        ex, ey = np.meshgrid(np.arange(xmin, xmax).astype(L) - L(x[j]), np.arange(ymin, ymax).astype(L) - L(y[j]))
        d2, r2 = ex * ex + ey * ey, L(r[j]) * L(r[j])
        best = min(best, float(np.min(np.abs(d2 - r2)) / r2) if r2 > 0 else (np.inf if np.min(d2) > 0 else 0.0))
    return best


def plain(v):
    """JSON-ready: numpy scalars to Python's, tuples and arrays to lists (a float round-trips through its repr bit for bit)."""
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    if isinstance(v, np.ndarray):
        return [plain(x) for x in v.tolist()]
    if isinstance(v, (np.floating, np.integer)):
        return v.item()
    return v


# ---- synthetic block files ---------------------------------------------------------------------------------------------------------------

def to_float64(primary32):
    """The float64 layers of a case with float64 PRIMARY: values that no float32 holds."""
    return primary32.astype(np.float64) * (1.0 + 2.0**-30)


def to_uint8(codes):
    """The uint8 codes of a case with uint8 FIDELITY."""
    return (codes.astype(np.int64) % 251).astype(np.uint8)


def synthetic_block(seed, nlayer, ny, nx):
    """(primary float32 [nlayer, ny, nx], fidelity uint16 [ny, nx] with zero codes, sigma int16 [ny, nx] with negative codes).  The layers
    hold eighths (few distinct bit patterns: the fixture stays small) and, in places, NaNs with payloads, infinities, -0.0 and subnormals."""
    rng = np.random.default_rng(seed)
    p = (rng.integers(-24, 24, size=(nlayer, ny, nx)) / 8.0).astype(np.float32)
    bits = p.view(np.uint32)
    special = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF], dtype=np.uint32)
    where = rng.random(p.shape) < 0.01
    bits[where] = special[rng.integers(0, len(special), size=int(where.sum()))]
    fid = rng.integers(1, 30000, size=40)[rng.integers(0, 40, size=(ny, nx))].astype(np.uint16)  # (forty codes a file)
    fid[rng.random((ny, nx)) < 0.03] = 0
    fid[rng.random((ny, nx)) < 0.01] = 65535
    sig = rng.integers(-3000, 3000, size=40)[rng.integers(0, 40, size=(ny, nx))].astype(np.int16)
    sig[rng.random((ny, nx)) < 0.01] = -32768
    return p, fid, sig
