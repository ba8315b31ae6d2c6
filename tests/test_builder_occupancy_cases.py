"""tests/builder_occupancy_cases.py checked on the CPU: the generated case contains the situations that
tests/test_gpu_builder_occupancy.py was written for -- read from the reference's own cell indices, so that an edit of the generator
cannot lose one silently."""

import numpy as np

from tests import builder_occupancy_cases as oc
from tests import builder_reference as br


def test_drift_case_has_both_row_loops_and_many_tiles():
    lds, glob = oc.drift_cases()
    refs = oc.drift_refs()
    ng = lds["geom"].ng
    assert lds["npsf_max"] == 4 <= 8 < glob["npsf_max"] == 9  # the pair table from LDS, and fetched per thread
    for k in ("n", "x", "y", "psf", "tables"):
        assert np.array_equal(lds[k], glob[k], equal_nan=True)
    assert np.array_equal(lds["pair_tab"], glob["pair_tab"][:, :4, :4]) and np.array_equal(lds["pair_pen"], glob["pair_pen"][:, :4, :4])
    assert lds["ldn"] == 256 and lds["n"].size == 16 and set(lds["n"]) == {17, 129, 200, 255}
    tiles = 0
    for s, (n, ref) in enumerate(zip(lds["n"], refs)):
        assert np.array_equal(lds["psf"][s, :n], np.arange(n) % 3) and (lds["psf"][s, n:] == 3).all()  # three PSFs interleaved
        nt = (int(n) + 15) // 16
        tiles += nt * (nt + 1) // 2
        # samples whose stencil ends on the last element of the stack (build_A_kernel's near_end): last table, cell (ng-6, ng-6)
        # unflipped, cell (4, 4) flipped
        last = ref.valid & (ref.code >= 0) & ((ref.code & br.PAIR_MASK) == oc.DRIFT_NTAB - 1)
        flip = (ref.code & br.PAIR_FLIP) != 0
        plain, flipped = last & ~flip & (ref.xi == ng - 6) & (ref.yi == ng - 6), last & flip & (ref.xi == 4) & (ref.yi == 4)
        if s in oc.DRIFT_STACK_END:
            assert plain[0, :16].any() and flipped[0, :16].any()  # the anchor's row of tile (0, 0) ...
            assert not (plain | flipped)[:16, :16].all() and ref.valid[:16, :16].sum() > 20  # ... among ordinary samples
        else:
            assert not (plain | flipped).any()
        assert ref.valid[np.triu_indices(int(n), 1)].mean() > 0.5  # most samples are on their table
    assert any((~x.valid & (x.code >= 0)).any() for x in refs) and any((x.code < 0).any() for x in refs)  # off the table; no table
    assert {int(lds["n"][s]) for s in oc.DRIFT_STACK_END} == {17, 129, 200, 255}
    assert tiles > 900  # tiles with samples in one launch (of 16 * 136 launched), both row loops among them
