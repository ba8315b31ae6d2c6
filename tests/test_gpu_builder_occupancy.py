"""build_A_kernel with every shared array inside its ring of stencil rows (four workgroups per CU): held to
tests/builder_reference.py exactly as tests/test_gpu_builder_edges.py holds it (its helpers are used as they are:
``|device - ref| <= K EPS (S + W + |pen|)`` per element, ``==`` for off-table samples, identity padding and symmetry), and to itself
from launch to launch.  tests/test_builder_occupancy_cases.py shows (on the CPU) that the case contains what is named here."""

import numpy as np
import pytest

from tests import builder_occupancy_cases as oc
from tests.test_gpu_builder_edges import _build_A, _check_A

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("P", [4, 9])
def test_build_A_aliased_ring_is_race_free(P):
    """16 stamps of n = 17, 129, 200, 255, three PSFs interleaved, four of them with stencils that end on the last element of the
    table stack: ~1000 tiles with samples in one launch, so that waves of different tiles share CUs and drift, the guarded row loop
    beside the plain one; the pair table from LDS (npsf_max = 4) and fetched per thread (9).  Against the reference, and three
    launches equal bit for bit: a race on an array that lives in the ring shows as a difference from run to run."""
    case = next(c for c in oc.drift_cases() if c["npsf_max"] == P)
    A = _build_A(case)
    _check_A(case, A, oc.drift_refs())
    for _ in range(2):
        assert np.array_equal(_build_A(case), A)
