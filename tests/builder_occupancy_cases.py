"""Inputs for tests/test_gpu_builder_occupancy.py, in the terms of tests/builder_reference.py (same reference, same bound).

build_A_kernel keeps every shared array inside its ring of stencil rows (four workgroups per CU): the case is one launch of many
tiles, with and without the guarded row loop, made to be run again and again.  tests/test_builder_occupancy_cases.py shows (on the
CPU) that it is."""

import functools

import numpy as np

from tests import builder_reference as br

DRIFT_N = (17, 129, 200, 255)
DRIFT_STACK_END = (1, 6, 11, 12)  # stamps (one of each size) whose tile (0, 0) reaches the end of the table stack
DRIFT_NTAB = 4


def _drift(P):
    """16 stamps of n = 17, 129, 200, 255 in turn, ldn = 256, three PSFs interleaved pixel by pixel and a fourth for the padding; in
    the stamps of DRIFT_STACK_END pixels 1, 4 (PSF 1) and 2, 5 (PSF 2) sit at the separations from pixel 0 (PSF 0) that end on the
    last element of the stack, plain and flipped (the construction of builder_reference's stack_end cases).  ``P`` is the side of
    the pair tables: their [:4, :4] corners, all that the pixels use, do not depend on it."""
    g = br.Geom(52, 0.5)
    ng = g.ng
    sep = lambda d: (d - g.nc - 6.0) * g.dscale
    rng = np.random.default_rng(7901)
    tables = br.make_tables(rng, DRIFT_NTAB, ng, smooth=(1,))
    xs, ys, psfs, tabs, pens = [], [], [], [], []
    for s in range(16):
        n = DRIFT_N[s % 4]
        x, y = br._q64(rng, 0.0, 14.25, n), br._q64(rng, 0.0, 14.25, n)
        tab4, pen4 = br._codes(4, DRIFT_NTAB, s)
        if s in DRIFT_STACK_END:
            tab4[0, 1], tab4[0, 2] = DRIFT_NTAB - 1, br.PAIR_FLIP | (DRIFT_NTAB - 1)
            x[0], y[0] = 6.0, 7.0
            for j, d in ((1, ng - 6.0), (4, ng - 6 + 0.75), (2, 4.0), (5, 4.96875)):
                x[j], y[j] = 6.0 - sep(d), 7.0 - sep(d)
        tab, pen = br._codes(P, DRIFT_NTAB, s + 3)
        tab[:4, :4], pen[:4, :4] = tab4, pen4
        xs.append(x), ys.append(y), psfs.append(np.arange(n) % 3), tabs.append(tab), pens.append(pen)
    return br._case_A(f"drift_P{P}", g, tables, xs, ys, psfs, 256, np.stack(tabs), np.stack(pens), 3)


@functools.lru_cache(maxsize=None)
def drift_cases():
    """The same pixels with the pair table in LDS (npsf_max = 4) and fetched per thread (npsf_max = 9)."""
    return _drift(4), _drift(9)


@functools.lru_cache(maxsize=None)
def drift_refs():
    """ref_A of every stamp: one reference for both pair-table sizes.  Computed once per process; nobody writes to it."""
    c = drift_cases()[0]
    return [br.ref_A(*br.stamp_A(c, s)) for s in range(c["n"].size)]
