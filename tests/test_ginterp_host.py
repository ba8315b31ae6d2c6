"""CPU-side checks of the pyimcom.meta.ginterp drop-in (pyimcom_amd/ginterp.py): the offset geometry against the reference's
(tests/golden/ginterp.npz, make_golden_ginterp.py), the public signatures, and the rule that picks the points of U / Sigma and of
Umax / Smax.  No device is used."""

import inspect

import numpy as np


def _corners(posx, posy, Rsearch):
    """The corner subsets as ginterp.py:157-159 selects them, in offset order."""
    R = np.sqrt(np.ceil(Rsearch**2) + 0.01)
    px, py = posx.astype(np.float64), posy.astype(np.float64)
    return [np.nonzero((px - xc) ** 2 + (py - yc) ** 2 <= R**2)[0] for xc, yc in [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0)]]


def test_geometry_matches_reference(golden):
    from pyimcom_amd import ginterp

    g = golden("ginterp")
    for name, Rs in [("a6", 6.0), ("a45", 4.5)]:
        posx, posy, corners = ginterp.geometry(Rs)
        assert posx.dtype == np.int16 and posy.dtype == np.int16
        assert np.array_equal(posx, g[f"{name}_posx"]) and np.array_equal(posy, g[f"{name}_posy"])
        ref = _corners(posx, posy, Rs)
        assert corners.shape == (4, ref[0].size)
        for c in range(4):
            assert np.array_equal(corners[c], ref[c])
    # the counts the kernel is built around (csrc/ginterp.hip): Rsearch 6 -> NN 140, n_g 113; Rsearch 8 -> 232, 197
    assert ginterp.geometry(6.0)[0].size == 140 and ginterp.geometry(6.0)[2].shape[1] == 113
    assert ginterp.geometry(8.0)[0].size == 232 and ginterp.geometry(8.0)[2].shape[1] == 197


def test_geometry_is_symmetric_about_the_cell():
    """Every corner subset is corner 0's shifted by the corner: the one factor of Ad[g0, g0] serves all four solves."""
    from pyimcom_amd import ginterp

    for Rs in (2.0, 4.5, 6.0, 7.3, 8.0):
        posx, posy, corners = ginterp.geometry(Rs)
        for c, (dx, dy) in enumerate([(0, 0), (1, 0), (0, 1), (1, 1)]):
            assert np.array_equal(posx[corners[c]] - dx, posx[corners[0]]) and np.array_equal(posy[corners[c]] - dy, posy[corners[0]])


def test_signatures_match_reference():
    from pyimcom_amd import ginterp

    s = inspect.signature(ginterp.InterpMatrix)
    assert list(s.parameters) == ["Rsearch", "samp", "x_out", "y_out", "Cov", "epsilon", "stest"]
    assert s.parameters["epsilon"].default == 1.0e-7 and s.parameters["stest"].default == 1
    s = inspect.signature(ginterp.MultiInterp)
    assert list(s.parameters) == ["in_array", "in_mask", "out_size", "out_origin", "out_transform", "Rsearch", "samp", "Cov", "epsilon", "stest",
                                  "blocksize"]
    assert s.parameters["epsilon"].default == 1.0e-7 and s.parameters["stest"].default == 1 and s.parameters["blocksize"].default == 393216


def test_stest_rule_follows_the_reference_chunk_loop():
    """Umax / Smax come from the points MultiInterp's chunk loop hands InterpMatrix at stride stest (ginterp.py:272-304)."""
    from pyimcom_amd import ginterp

    for npts, stest, bs in [(3600, 2, 1000), (1000, 3, 1000), (10, 1, 393216), (2503, 7, 250), (17, 4, 5)]:
        want = []
        istart = 0
        while istart < npts:
            ngroup = min(bs, npts - istart)
            want.extend(range(istart, istart + ngroup)[::stest])
            istart += bs
        assert np.array_equal(ginterp.stest_points(npts, stest, bs), np.array(want))
    assert np.array_equal(ginterp.stest_points(10, 3), np.array([0, 3, 6, 9]))


def test_unsupported_dtype_is_refused():
    import pytest

    from pyimcom_amd import ginterp

    with pytest.raises(TypeError):
        ginterp.MultiInterp(np.zeros((40, 40), dtype=np.int32), np.zeros((40, 40), dtype=bool), (4, 4), [10, 10], np.identity(2), 4.5, 5.0,
                            [0.1, 0, 0.1])


def test_geometry_refuses_bad_radius():
    """A NaN or a far-off Rsearch (the offset grid grows as Rsearch^2) is refused before any grid is built."""
    import pytest

    from pyimcom_amd import _lib, ginterp

    for Rs in (float("nan"), float("inf"), 0.0, -3.0, 1.0e5):
        with pytest.raises(_lib.ImcomError):
            ginterp.geometry(Rs)
