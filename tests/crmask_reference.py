"""A plain-integer restatement of what csrc/pcg64.hip computes: numpy's PCG64 stream by position and the cosmic-ray mask of
``Mask.randmask`` (reference src/pyimcom/layer.py:933-964) made of it.  Python ints only -- no numpy in the arithmetic -- so it is
slow and obviously exact; tests/test_crmask_host.py pins it to numpy's ``Generator.uniform`` and to the reference's own outputs
(tests/golden/crmask.npz)."""

import numpy as np

MULT = 0x2360ED051FC65DA44385DF649FCCF645  # PCG_DEFAULT_MULTIPLIER_128
M128 = (1 << 128) - 1
M64 = (1 << 64) - 1
PAD, N_SLICES, SEED0 = 10, 18, 100000000  # layer.py:954-957


def stream(seed_or_bitgen):
    """(state, inc) as numpy reports them; seeding is numpy's."""
    bg = seed_or_bitgen if isinstance(seed_or_bitgen, np.random.PCG64) else np.random.PCG64(seed_or_bitgen)
    st = bg.state["state"]
    return int(st["state"]), int(st["inc"])


def jump_maps(inc):
    """[(A_j, C_j)], j < 128: s -> A_j s + C_j is 2^j steps of s -> MULT s + inc."""
    maps, A, C = [], MULT, inc
    for _ in range(128):
        maps.append((A, C))
        A, C = (A * A) & M128, ((A + 1) * C) & M128
    return maps


def jump(state, inc, d, maps=None):
    """The state d steps on: one affine map per set bit of d."""
    maps = maps or jump_maps(inc)
    d &= M128
    j = 0
    while d:
        if d & 1:
            state = (maps[j][0] * state + maps[j][1]) & M128
        d >>= 1
        j += 1
    return state


def output(state):
    """XSL-RR: the high and low halves xor-ed, rotated right by the top six bits; then the 53-bit double."""
    x = ((state >> 64) ^ state) & M64
    rot = state >> 122
    out = ((x >> rot) | (x << ((64 - rot) & 63))) & M64
    return (out >> 11) * 2.0**-53


def uniform_at(state, inc, k, maps=None):
    """U[k]: the output of the state after k + 1 steps."""
    return output((MULT * jump(state, inc, k, maps) + inc) & M128)


def uniform(state, inc, offset, count):
    """[U[offset], .., U[offset + count - 1]]: one jump, then steps."""
    s = jump(state, inc, offset)
    out = []
    for _ in range(count):
        s = (MULT * s + inc) & M128
        out.append(output(s))
    return out


def hit_rows(state, inc, nside, sca_slice, pcut, rows, pad=PAD, maps=None):
    """{r: [hit of padded pixel (r, c) for c = pad - 1 .. pad + nside]} for the padded rows asked for."""
    W = nside + 2 * pad
    maps = maps or jump_maps(inc)
    out = {}
    for r in rows:
        out[r] = [u < pcut for u in uniform(jump(state, inc, sca_slice * W * W + r * W + pad - 1, maps), inc, 0, nside + 2)]
    return out


def mask_rows(seed, nside, sca_slice, pcut, ys, pad=PAD):
    """Rows ``ys`` of the mask, bool [len(ys), nside]: good where none of the nine padded pixels around (y + pad, x + pad) is a hit."""
    state, inc = stream(seed)
    need = sorted({y + pad + dy for y in ys for dy in (-1, 0, 1)})
    hits = hit_rows(state, inc, nside, sca_slice, pcut, need, pad)
    out = np.zeros((len(ys), nside), dtype=bool)
    for i, y in enumerate(ys):
        col = [hits[y + pad - 1][c] or hits[y + pad][c] or hits[y + pad + 1][c] for c in range(nside + 2)]
        out[i] = [not (col[x] or col[x + 1] or col[x + 2]) for x in range(nside)]
    return out


def randmask(idsca, pcut, nside, pad=PAD):
    """``Mask.randmask(idsca, pcut)`` with ``Stn.sca_nside = nside``."""
    return mask_rows(SEED0 + int(idsca[0]), nside, int(idsca[1]) - 1, pcut, list(range(nside)), pad)


def subgen_multirow(state, inc, lenpix, subpix, P):
    """``GalSimInject.subgen_multirow``: out[j][i] = U[j lenpix + subpix[i]]; and the state P lenpix steps on."""
    maps = jump_maps(inc)
    out = np.array([[uniform_at(state, inc, j * lenpix + int(p), maps) for p in subpix] for j in range(P)]).reshape(P, len(subpix))
    return out, jump(state, inc, P * lenpix, maps)
