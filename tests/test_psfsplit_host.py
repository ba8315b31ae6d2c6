"""The numpy restatement of PSFSPLIT's coaddition stage (tests/psfsplit_reference.py) against the reference's own outputs
(tests/golden/psfsplit.npz, make_golden_psfsplit.py), and the host-side contract of the Block seam's ``psfsplit`` keyword.  No GPU."""

import numpy as np
import pytest

from oracle import oracle as orc
from tests import psfsplit_reference as psr


class Empty:
    pass


def _geom(g, tag):
    npixpsf, oversamp, ns, nfft, ntab = (int(v) for v in g[f"{tag}_pars"])
    sg = psr.SplitGeom(npixpsf, oversamp, 0.04 / 3600.0, 1e-7)
    assert (sg.psf.nsamp, sg.psf.nfft, sg.tab.nsamp, sg.tab.nc) == (ns, nfft, ntab, ns) and sg.psf.dscale == float(g[f"{tag}_dscale"])
    return sg


def test_wide_tables_bit_for_bit(golden):
    """PSFOvl's tables under psfsplit (psfutil.py:1087-1089, 1226-1227) for both geometries of the fixture: transforms, self, cross and
    input-output tables and C equal the reference's arrays bit for bit; the central nsamp x nsamp window of a wide table is the unsplit
    table of the same PSFs bit for bit (the same irfft2)."""
    g = golden("psfsplit")
    for tag in "ab":
        sg = _geom(g, tag)
        ns = sg.psf.nsamp
        r1, r2, ro = (orc.pad_and_rfft2(g[f"{tag}_{k}"], sg.psf) for k in ("psf1", "psf2", "psfo"))
        o_self, o_cross, o_io = orc.overlap_self(r1, sg.tab), orc.overlap_cross(r1, r2, sg.tab), orc.overlap_cross(r1, ro, sg.tab)
        assert o_self.shape == (6, 2 * ns + 1, 2 * ns + 1)
        assert np.array_equal(o_io, g[f"{tag}_ovl_io"]) and np.array_equal(orc.overlap_out_C(ro, sg.tab), g[f"{tag}_outovlc"])
        if tag == "a":
            assert np.array_equal(r1[0], g["a_rft1_0"]) and np.array_equal(o_self, g["a_ovl_self"]) and np.array_equal(o_cross[[0, 2]], g["a_ovl_cross_02"])
        else:
            assert np.array_equal(o_self[:3], g["b_ovl_self_0"])
        lo = ns - ns // 2
        assert np.array_equal(o_cross[:, :, lo : lo + ns, lo : lo + ns], orc.overlap_cross(r1, r2, sg.psf))
    # the stack order of the device's PSFGroupTables
    tabs, C = psr.table_set(g["a_psf1"], g["a_psfo"], _geom(g, "a"))
    assert np.array_equal(tabs[:6], g["a_ovl_self"]) and np.array_equal(tabs[6:], g["a_ovl_io"][:, 0]) and np.array_equal(C, g["a_outovlc"])


def test_wide_tables_amp_penalty(golden):
    """cfg.amp_penalty (psfutil.py:661-671) through to a wide table and C: the reference reweights the transforms in place, the
    restatement multiplies copies -- the same products, bit for bit."""
    g = golden("psfsplit")
    sg = _geom(g, "a")
    ns, ov = sg.psf.nsamp, sg.psf.oversamp
    a0, a1 = g["amp_penalty"]
    mk = lambda kind, sig: orc.finish_psf_group(orc.sample_psf(orc.get_outpsf(kind, sig, 2, ns, ov), ns)[None].copy(), True, True)  # noqa: E731
    tabs, C = psr.table_set(mk("GAUSSIAN", float(g["amp_targets"][0])), mk("AIRYOBSC", float(g["amp_targets"][1])), sg, amp=(a0, a1 * ov))
    assert np.array_equal(tabs[1], g["amp_ovl_io"][0, 0]) and np.array_equal(C, g["amp_outovlc"])


def test_wide_subblocks_bit_for_bit(golden):
    """PSFOvl.__call__ on wide tables (_call_ii_self 1597-1732, _call_ii_cross 1401-1495, _call_io_cross 1497-1595) for InStamps whose
    separations lie off the unsplit table: bit for bit, as tests/test_oracle.py pins the unsplit sub-blocks."""
    g = golden("psfsplit")
    sg = _geom(g, "a")
    r1, r2, ro = (orc.pad_and_rfft2(g[f"a_{k}"], sg.psf) for k in ("psf1", "psf2", "psfo"))
    o_self, o_cross, o_io = orc.overlap_self(r1, sg.tab), orc.overlap_cross(r1, r2, sg.tab), orc.overlap_cross(r1, ro, sg.tab)
    c1, c2 = g["st1_count"], g["st2_count"]
    s1, s2 = (g["st1_x"], g["st1_y"], c1), (g["st2_x"], g["st2_y"], c2)
    A11 = orc.subblock_ii_self(o_self, 3, sg.tab, *s1)
    assert np.array_equal(A11, g["A_self_11"]) and np.array_equal(A11, A11.T)
    A12, X12 = orc.subblock_ii_self(o_self, 3, sg.tab, *s1, *s2), orc.subblock_ii_cross(o_cross, sg.tab, *s1, *s2)
    assert np.array_equal(A12, g["A_self_12"]) and np.array_equal(X12, g["A_cross_12"])
    ox, oy = g["out_yx"][1, 0, :], g["out_yx"][0, :, 0]
    assert np.array_equal(orc.subblock_io(o_io, sg.tab, *s1, ox, oy), g["B_io_1all"])
    assert np.array_equal(orc.subblock_io(o_io, sg.tab, *s1, ox, oy, g["sel1"].astype(int)), g["B_io_1sel"])
    # the separations really need the wide table: on the unsplit one (same PSFs) a part of every cross sub-block falls off the grid
    narrow = orc.subblock_ii_cross(orc.overlap_cross(r1, r2, sg.psf), sg.psf, *s1, *s2)
    assert np.abs(narrow - X12).max() > 1e-9 * np.abs(X12).max()


def test_affine_positions_and_sampling_bit_for_bit(golden):
    """PSFGrp._sample_psf, psfsplit branch (psfutil.py:739-753), on a map that is not affine: cardinal points, positions (captured where
    the reference hands them to its interpolator) and sampled PSFs, bit for bit."""
    g = golden("psfsplit")
    sg = _geom(g, "a")
    p0 = tuple(g["samp_p0"])
    for e in range(2):
        M, t0, q = g["samp_M"][e], g["samp_t0"][e], float(g["samp_q"][e])

        def f(xy):
            xy = np.asarray(xy, dtype=np.float64)
            d = xy - np.array(p0)
            return xy @ M.T + t0 + q * np.stack([d[:, 0] * d[:, 1], d[:, 0] ** 2 - d[:, 1] ** 2], axis=1)

        card = psr.cardinal_points(f, p0, sg.psf.oversamp, sg.psf.dscale)
        assert np.array_equal(card, g["samp_cardinal"][e])
        co = psr.affine_yxco(card, sg.psf.yxo)
        assert np.array_equal(co, g["samp_yxco"][e])
        assert np.array_equal(orc.sample_psf(g["samp_psf"][e], sg.psf.nsamp, co), g["samp_psf_arr"][e])


def test_host_cardinal_points_match_the_restatement(golden):
    """pyimcom_amd.psfs.cardinal_points (the host half of the device's affine positions) is the restatement's, bit for bit."""
    from pyimcom_amd import psfs

    g = golden("psfsplit")
    sg = _geom(g, "a")
    M, t0 = g["samp_M"][0], g["samp_t0"][0]
    f = lambda xy: np.asarray(xy) @ M.T + t0  # noqa: E731
    assert np.array_equal(psfs.cardinal_points(f, g["samp_p0"], sg.psf.oversamp, sg.psf.dscale), psr.cardinal_points(f, g["samp_p0"], sg.psf.oversamp, sg.psf.dscale))


def test_psfsplit_is_opt_in():
    """``check_supported``: a PSFSPLIT configuration is refused without the keyword (status IMCOM_ERR_UNSUPPORTED, the message names the
    keyword), accepted with it; the keyword on a configuration without PSFSPLIT is an error, not a guess."""
    from pyimcom_amd._lib import ImcomError
    from pyimcom_amd.refblock import IMCOM_ERR_UNSUPPORTED, check_supported

    cfg = Empty()
    cfg.linear_algebra, cfg.psfsplit = "Cholesky", [3.0, 6.0, 1e-3]
    with pytest.raises(ImcomError) as ei:
        check_supported(cfg)
    assert ei.value.status == IMCOM_ERR_UNSUPPORTED and "psfsplit=True" in str(ei.value)
    check_supported(cfg, psfsplit=True)
    plain = Empty()
    plain.linear_algebra = "Cholesky"
    with pytest.raises(ValueError):
        check_supported(plain, psfsplit=True)
    cfg.psf_interp = "G4460"  # the other refusals stand under the keyword
    with pytest.raises(ImcomError):
        check_supported(cfg, psfsplit=True)

