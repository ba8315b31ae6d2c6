"""A numpy restatement of the sharing of padding stamps between neighbouring blocks (seam 20): the reference's
``OutImage._update_hdu_data`` (src/pyimcom/analysis.py:394-537), ``get_output_map`` (344-392) and the loop of
``Mosaic.share_padding_stamps`` (1429-1467), written from their description.  tests/golden/make_golden_padshare.py asserts that it gives
what the reference's own statements give, bit for bit; the tests compare the device with it where the fixture holds no recorded answer.

A block is a dict: ``primary`` float32 [n_out, nlayer, NsideP, NsideP], ``inweight`` float32 [n_out, n_inimage, n1P, n1P], ``idscas`` a list of
(obsid, sca), ``maps`` a dict name -> [codes (u)int16 [n_out, NsideP, NsideP], unit, comment] in file order.  ``update`` changes ``mine`` in
place and returns the float32 sums of every map strip before the encode."""

import re

import numpy as np

DIRECTIONS = ("left", "right", "bottom", "top")
# coadd.py:2247-2305: HDU name -> (outmaps letter, encode coefficient, dtype, UNIT value, UNIT comment)
MAPS = {"FIDELITY": ("U", -5000, np.uint16, "-0.2mB", "-5000*log10(U/C)"), "SIGMA": ("S", -10000, np.int16, "-0.1mB", "-10000*log10(Sigma)"),
        "KAPPA": ("K", -5000, np.uint16, "-0.2mB", "-5000*log10(kappa)"), "INWTSUM": ("T", 200000, np.int16, "5uB", "200000*log10(Tsum)"),
        "EFFCOVER": ("N", 50000, np.uint16, "20uB", "50000*log10(Neff)")}


def unit_to_bels(unit, comment):
    """helper.py:19-82: the UNIT value in bels, negated for a legacy file whose comment starts with '-' while the value is positive."""
    s = re.match(r"([\d\.\-\+eE]+)([mun]?)B", unit)
    if not s:
        return np.nan
    x = float(s.group(1))
    if s.group(2) == "m":
        x *= 1e-3
    if s.group(2) == "u":
        x *= 1e-6
    if s.group(2) == "n":
        x *= 1e-9
    if x > 0 and comment[0] == "-":
        x = -x
    return x


def code_range(dtype):
    return (0, 65535) if np.dtype(dtype) == np.dtype("uint16") else (-32768, 32767)


def decode(codes, unit, comment, zero_floor=None):
    """get_output_map(outmap, None).  zero_floor None: line 387 as the installed numpy evaluates it; True: the comparison scalar is cast to
    float32 (numpy < 2: every floor code becomes 0); False: nothing is zeroed."""
    coef = 1.0 / unit_to_bels(unit, comment)
    data = np.power(10.0, codes / coef).astype(np.float32)
    a_min, a_max = code_range(codes.dtype)
    a_zero = a_min if coef > 0 else a_max
    floor = np.power(10.0, a_zero / coef)
    if zero_floor is None:
        data[data == floor] = 0.0
    elif zero_floor:
        data[data == np.float32(floor)] = 0.0
    return data


def taper(fk):
    s = np.arange(1, 2 * fk + 1, dtype=np.float64) / (2 * fk + 1)
    return s - np.sin(2 * np.pi * s) / (2 * np.pi)


def compress(map_, coef, dtype):
    a_min, a_max = code_range(dtype)
    return np.clip(np.floor(coef * np.log10(np.clip(map_, 1e-32, None)) + 0.5), a_min, a_max).astype(dtype)


def compress_device(map_, coef, dtype):
    """The device's encode: log10 correctly rounded to float32 (formed in double), the product and the sum in float32."""
    a_min, a_max = code_range(dtype)
    lg = np.log10(np.clip(map_, np.float32(1e-32), None).astype(np.float64)).astype(np.float32)
    return np.clip(np.floor(np.float32(coef) * lg + np.float32(0.5)), a_min, a_max).astype(dtype)


def strips(direction, n, w, fk):
    """(my, ur): the index ranges along the strip axis (435-446; INWEIGHT: n1P, pad, 0)."""
    if direction in ("left", "bottom"):
        return slice(0, w + fk), slice(n - 2 * w, n - w + fk)
    return slice(n - w - fk, n), slice(w - fk, 2 * w)


def pairs(my_idscas, ur_idscas):
    """468-470: (my_idx, ur_idx) of every (obsid, sca) both lists hold, first occurrences, sorted by my_idx."""
    my, ur = [tuple(x) for x in my_idscas], [tuple(x) for x in ur_idscas]
    return sorted((my.index(x), ur.index(x)) for x in set(my) & set(ur))


def update(mine, theirs, direction, add_mode, n2, postage_pad, fk, zero_floor=None, encode=compress):
    assert direction in DIRECTIONS
    NsideP, n1P = mine["primary"].shape[-1], mine["inweight"].shape[-1]
    width, pad = postage_pad * n2, postage_pad
    along_x = direction in ("left", "right")
    at = (lambda s: np.s_[..., :, s]) if along_x else (lambda s: np.s_[..., s, :])
    my, ur = strips(direction, NsideP, width, fk)
    with np.errstate(invalid="ignore"):  # (inf * False)
        mine["primary"][at(my)] = mine["primary"][at(my)] * add_mode + theirs["primary"][at(ur)]
    wmy, wur = strips(direction, n1P, pad, 0)
    for i, j in pairs(mine["idscas"], theirs["idscas"]):
        mine["inweight"][(slice(None), i) + at(wmy)[1:]] = theirs["inweight"][(slice(None), j) + at(wur)[1:]]
    sums = {}
    for name, (codes, unit, comment) in mine["maps"].items():
        my_maps = decode(codes, unit, comment, zero_floor)
        ur_maps = decode(theirs["maps"][name][0], theirs["maps"][name][1], theirs["maps"][name][2], zero_floor)
        if add_mode and fk > 0:
            s = taper(fk)
            rise, fall = slice(width - fk, width + fk), slice(NsideP - width + fk - 1, NsideP - width - fk - 1, -1)
            sh = s if along_x else s[:, None]
            my_maps[at(rise if direction in ("left", "bottom") else fall)] *= sh
            ur_maps[at(fall if direction in ("left", "bottom") else rise)] *= sh
        coef = int(comment.partition("*")[0])
        sums[name] = my_maps[at(my)] * add_mode + ur_maps[at(ur)]
        codes[at(my)] = encode(sums[name], coef, codes.dtype.newbyteorder("="))
    return sums


def inwtflat(inweight):
    n_out, n_in, n1P = inweight.shape[:3]
    return np.transpose(inweight, axes=(0, 2, 1, 3)).reshape((n_out * n1P, n_in * n1P))


def share_order(nblock):
    """The calls of share_padding_stamps in order: ("load" | "save", iby, ibx) and ("update", (iby, ibx) of mine, of theirs, direction, add)."""
    out = []
    for iby in range(nblock):
        out.append(("load", iby, 0))
        for ibx in range(nblock - 1):
            out.append(("load", iby, ibx + 1))
            out.append(("update", (iby, ibx), (iby, ibx + 1), "right", True))
            out.append(("update", (iby, ibx + 1), (iby, ibx), "left", False))
            out.append(("save", iby, ibx))
        out.append(("save", iby, nblock - 1))
    for ibx in range(nblock):
        out.append(("load", 0, ibx))
        for iby in range(nblock - 1):
            out.append(("load", iby + 1, ibx))
            out.append(("update", (iby, ibx), (iby + 1, ibx), "top", True))
            out.append(("update", (iby + 1, ibx), (iby, ibx), "bottom", False))
            out.append(("save", iby, ibx))
        out.append(("save", nblock - 1, ibx))
    return out


def share_padding_stamps(blocks, n2, postage_pad, fk, zero_floor=None, encode=compress):
    for step in share_order(len(blocks)):
        if step[0] == "update":
            (ay, ax), (by, bx) = step[1], step[2]
            update(blocks[ay][ax], blocks[by][bx], step[3], step[4], n2, postage_pad, fk, zero_floor, encode)


def copy_block(b):
    return {"primary": b["primary"].copy(), "inweight": b["inweight"].copy(), "idscas": list(b["idscas"]),
            "maps": {k: [v[0].copy(), v[1], v[2]] for k, v in b["maps"].items()}}


# ---- tests/golden/padshare.npz ------------------------------------------------------------------------------------------------------------

def fixture_block(G, prefix, units, idscas):
    """The block whose arrays the fixture holds under ``prefix``; ``units``: name -> (unit, comment) in file order."""
    return {"primary": G[prefix + "_primary"].copy(), "inweight": G[prefix + "_inweight"].copy(), "idscas": [tuple(p) for p in idscas],
            "maps": {k: [G[f"{prefix}_{k}"].copy(), u, c] for k, (u, c) in units.items() if f"{prefix}_{k}" in G}}


def same_bits(a, b):
    """array_equal on the bit patterns (sign of zero included), NaN matching NaN; the byte order is no part of the value."""
    a, b = (np.ascontiguousarray(v.astype(v.dtype.newbyteorder("="))) for v in (np.asarray(a), np.asarray(b)))
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    view = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.all((a.view(view) == b.view(view)) | (np.isnan(a) & np.isnan(b))))


def strip_of(a, direction, s):
    return a[..., :, s] if direction in ("left", "right") else a[..., s, :]
