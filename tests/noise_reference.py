"""numpy's float64 normal draw restated over the raw 64-bit outputs of the bit generator, in plain integers and libm calls (``math.exp``,
``math.log1p``: the functions numpy's C code calls), and the crafting of PCG64 states whose next output is a chosen word.  The tables are
parsed from pyimcom_amd/csrc/ziggurat_tables.h."""

import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZIG_R, ZIG_INV_R = 3.6541528853610088, 0.27366123732975828
MULT = 0x2360ED051FC65DA44385DF649FCCF645
M128, M64 = (1 << 128) - 1, (1 << 64) - 1
MASK52 = (1 << 52) - 1
FAST, WEDGE, REJECT, TAIL = 0, 1, 2, 3


def tables():
    """(wi float64 [256], ki uint64 [256], fi float64 [256]) of the committed header."""
    text = open(os.path.join(ROOT, "pyimcom_amd", "csrc", "ziggurat_tables.h")).read()
    out = []
    for name in ("ZIG_WI", "ZIG_KI", "ZIG_FI"):
        body = re.search(name + r"\[256\] = \{(.*?)\};", text, re.S).group(1)
        items = [t.strip() for t in body.split(",") if t.strip()]
        assert len(items) == 256
        out.append(np.array([int(t[:-3], 16) for t in items], dtype=np.uint64) if name == "ZIG_KI" else np.array([float.fromhex(t) for t in items]))
    return tuple(out)


def word(idx, sign, rabs):
    return (rabs << 9) | (sign << 8) | idx


def crafted_pcg64(words_first, inc=None):
    """A PCG64 whose next output is ``words_first``: hi is free (0 here, so the rotation is 0 and lo = the word), and the state is one
    LCG step back, through the multiplier's inverse mod 2^128."""
    bg = np.random.PCG64(0)
    st = bg.state
    inc = st["state"]["inc"] if inc is None else inc
    hi = 0
    after = (hi << 64) | (hi ^ int(words_first))  # rot = hi >> 58 = 0
    before = ((after - inc) * pow(MULT, -1, 1 << 128)) & M128
    st["state"] = {"state": before, "inc": inc}
    bg.state = st
    return bg


def attempt(raw, k, wi, ki, fi):
    """(kind, outputs consumed, value) of the attempt starting at raw[k]; raw: a sequence of Python ints."""
    w = int(raw[k])
    idx, sign, rabs = w & 0xFF, (w >> 8) & 1, (w >> 9) & MASK52
    x = rabs * float(wi[idx])
    if sign:
        x = -x
    if rabs < int(ki[idx]):
        return FAST, 1, x
    if idx == 0:
        used = 1
        while True:
            xx = -ZIG_INV_R * math.log1p(-((int(raw[k + used]) >> 11) * 2.0**-53))
            yy = -math.log1p(-((int(raw[k + used + 1]) >> 11) * 2.0**-53))
            used += 2
            if yy + yy > xx * xx:
                return TAIL, used, -(ZIG_R + xx) if (rabs >> 8) & 1 else ZIG_R + xx
    u = (int(raw[k + 1]) >> 11) * 2.0**-53
    if (float(fi[idx - 1]) - float(fi[idx])) * u + float(fi[idx]) < math.exp(-0.5 * x * x):
        return WEDGE, 2, x
    return REJECT, 2, x


def normals_from_raw(raw, count, tabs):
    """(draws float64 [count], outputs consumed, events): the chain of attempts from raw[0].  events: (position, kind, consumed, draw index)
    of every attempt on the chain that left the fast path.  Runs of fast attempts are copied as arrays; the others are walked one by one."""
    wi, ki, fi = tabs
    raw = np.asarray(raw, dtype=np.uint64)
    idx = (raw & np.uint64(0xFF)).astype(np.int64)
    rabs = (raw >> np.uint64(9)) & np.uint64(MASK52)
    x = rabs.astype(np.float64) * wi[idx]
    x = np.where((raw >> np.uint64(8)) & np.uint64(1), -x, x)
    slow = np.flatnonzero(rabs >= ki[idx])
    out, n, c, j, events = np.empty(count), 0, 0, 0, []
    while n < count:
        while j < len(slow) and slow[j] < c:
            j += 1
        s = int(slow[j]) if j < len(slow) else len(raw)
        take = min(s - c, count - n)
        out[n:n + take] = x[c:c + take]
        n, c = n + take, c + take
        if n == count:
            break
        if s >= len(raw):
            raise ValueError("not enough outputs")
        kind, used, val = attempt(raw, s, wi, ki, fi)
        events.append((s, kind, used, n))
        if kind != REJECT:
            out[n] = val
            n += 1
        c = s + used
    return out, c, events
