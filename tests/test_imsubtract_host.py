"""Host side of pyimcom_amd.imsubtract (no GPU): the geometry, the phase tables, prepare_kernel and the byte plan, and the numpy / scipy
restatement tests/imsubtract_reference.py pinned to what the reference's own code produced (tests/golden/imsubtract.npz,
tests/golden/make_golden_imsubtract.py)."""

import os

import numpy as np
import pytest

from tests import imsubtract_reference as ref
from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "imsubtract.npz")
CASES = ["a", "b", "c", "d", "e"]
F32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def ims():
    import __graft_entry__ as g

    g.build()
    from pyimcom_amd import imsubtract

    return imsubtract


def _pars(gold, name):
    nside, s, ax, ncoeff, porder, Nl, I_pad, first, A = (int(v) for v in gold[f"{name}_pars"])
    return dict(nside=nside, s=s, ax=ax, ncoeff=ncoeff, porder=porder, Nl=Nl, I_pad=I_pad, first=first, A=A)


def test_golden_holds_the_cases_of_the_issue(gold):
    assert list(gold["cases"]) == CASES
    a, b = _pars(gold, "a"), _pars(gold, "b")
    assert (a["nside"], a["s"], a["ax"], a["Nl"], a["A"]) == (48, 4, 40, 2, 232)
    assert (b["nside"], b["s"], b["ax"], b["ncoeff"], b["Nl"]) == (32, 8, 48, 16, 3)
    assert not gold["c_canvas"][:46].any() and gold["c_canvas"][46:].any()  # whole zero bands
    for name in CASES:
        assert 0.0 < float(gold[f"{name}_ref_err"]) < 1.0e-6  # a few float32 roundings


@pytest.mark.parametrize("name", CASES)
def test_geometry_and_order_match_the_reference(gold, ims, name):
    p = _pars(gold, name)
    assert ims.geometry(p["ax"], p["s"], p["nside"]) == (p["I_pad"], p["first"], p["A"]) == ref.geometry(p["ax"], p["s"], p["nside"])
    assert ims.legendre_order(p["ncoeff"], p["porder"]) == p["Nl"]
    from pyimcom_amd._lib import lib, ptr

    sz = np.zeros(6, dtype=np.int64)
    assert lib.imcom_imsub_sizes(p["ax"], p["s"], p["nside"], p["Nl"], ptr(sz)) == 0
    npk = p["ax"] // p["s"]
    assert list(sz) == [p["I_pad"], p["first"], p["A"], npk, -(-npk // 8) * 8, p["Nl"] ** 2 * p["s"] ** 2 * npk * (-(-npk // 8) * 8)]


def test_bad_shapes_are_refused_on_the_host(ims):
    from pyimcom_amd._lib import lib, ptr

    sz = np.zeros(6, dtype=np.int64)
    for ax, s in ((40, 8), (44, 8), (9, 4), (4, 8)):
        with pytest.raises(ValueError):
            ims.geometry(ax, s, 32)
        assert lib.imcom_imsub_sizes(ax, s, 32, 1, ptr(sz)) == -1
        assert b"axis_num" in lib.imcom_last_error()
    with pytest.raises(ValueError):
        ims.legendre_order(8, 3)  # 9 planes out of 8
    assert ims.legendre_order(16, -1) == 4 and ims.legendre_order(15, -1) == 3 and ims.legendre_order(16, 0) == 0


@pytest.mark.parametrize("name", CASES)
def test_phase_tables_against_the_brute_force_sum(gold, ims, name):
    """Output row Y and flipped kernel row jj of phase p meet at canvas row s (Y + B[p] + jj) + rho[p]: the sum rebuilt from the tables
    alone equals the defining sum, and every index stays inside the canvas."""
    p = _pars(gold, name)
    s, ax, nside, Nl, A = p["s"], p["ax"], p["nside"], p["Nl"], p["A"]
    rho, B = ims.phase_tables(ax, s, p["first"])
    npk = ax // s
    assert rho.min() >= 0 and rho.max() < s and sorted(rho) == list(range(s)) and B.min() >= 0
    assert s * (nside - 1 + B.max() + npk - 1) + rho.max() < A
    canvas, K = gold[f"{name}_canvas"], gold[f"{name}_K"]
    u = ref.u_canvas(ax, s, nside)
    samples = [(0, 0), (nside - 1, nside - 1), (nside // 2, 3), (1, nside - 2)]
    want = ref.kh_brute(canvas, K, s, nside, Nl, samples)
    got = np.zeros(len(samples))
    for lu in range(Nl):
        for lv in range(Nl):
            arr = ref.modulated(canvas, u, lu, lv).astype(np.float64)
            Kc = K[lu + lv * Nl].astype(np.float64)
            for pp in range(s):
                for q in range(s):
                    Kf = Kc[pp::s, q::s][::-1, ::-1]
                    for k, (Y, X) in enumerate(samples):
                        rows = s * (Y + B[pp] + np.arange(npk)) + rho[pp]
                        cols = s * (X + B[q] + np.arange(npk)) + rho[q]
                        got[k] += np.sum(Kf * arr[np.ix_(rows, cols)])
    assert np.abs(got - want).max() <= 1.0e-12 * np.abs(gold[f"{name}_kh64"]).max()


@pytest.mark.parametrize("name", CASES)
def test_restatement_is_pinned_to_the_golden(gold, name):
    """The float64 restatements (full resolution and by phases) agree with the generator's float64 evaluation to float64 rounding, the
    float32-accumulating one with the reference's KH to the reference's own error, and a brute-force sum with both."""
    p = _pars(gold, name)
    canvas, K, kh64, kh_ref = gold[f"{name}_canvas"], gold[f"{name}_K"], gold[f"{name}_kh64"], gold[f"{name}_kh_ref"]
    top, ref_err = np.abs(kh64).max(), float(gold[f"{name}_ref_err"])
    full = ref.kh_full(canvas, K, p["s"], p["nside"], p["Nl"])
    phases = ref.kh_phases(canvas, K, p["s"], p["nside"], p["Nl"])
    assert full.shape == kh64.shape == phases.shape
    assert np.abs(full - kh64).max() <= 1.0e-13 * top
    assert np.abs(phases - kh64).max() <= 1.0e-12 * top
    samples = [(0, 0), (p["nside"] - 1, 0), (p["nside"] // 3, p["nside"] // 2)]
    brute = ref.kh_brute(canvas, K, p["s"], p["nside"], p["Nl"], samples)
    assert np.abs(brute - np.array([kh64[y, x] for y, x in samples])).max() <= 1.0e-12 * top
    assert np.abs(kh_ref.astype(np.float64) - kh64).max() == pytest.approx(ref_err * top, rel=1e-6)
    f32 = ref.kh_full(canvas, K, p["s"], p["nside"], p["Nl"], dtype=np.float32)
    assert np.abs(f32.astype(np.float64) - kh_ref).max() <= 2.0 * ref_err * top
    # the subtracted layer: the reference rounds KH and the difference, the restatement the difference alone
    image, sub_ref = gold[f"{name}_image"], gold[f"{name}_sub_ref"]
    assert np.array_equal(sub_ref, image - kh_ref)
    assert np.abs(ref.subtract(image, kh64).astype(np.float64) - sub_ref).max() <= ref_err * top + F32 * np.abs(image).max()


@pytest.mark.parametrize("name", ["prep_pad", "prep_trim"])
def test_prepare_kernel_against_the_golden(gold, ims, name):
    """Both branches of imsubtract.py:373-378.  The reference re-interpolates in float32 (a 16-term sum of float32 products, scipy's direct
    convolution), prepare_kernel in float64 rounded once: they may differ by the float32 error of that sum, bounded here by 16 roundings of
    the largest product (weights up to 1.125^2)."""
    K0, (s0, s1, ax1), want = gold[f"{name}_K0"], gold[f"{name}_pars"], gold[f"{name}_K"]
    got, s = ims.prepare_kernel(K0, int(s0), bin2x2=True)
    assert s == int(s1) and got.shape == want.shape == (K0.shape[0], int(ax1), int(ax1)) and got.dtype == np.float32
    assert np.abs(got.astype(np.float64) - want).max() <= 16 * 1.125**2 * (F32 / 2) * np.abs(K0).max()
    same, s_same = ims.prepare_kernel(K0, int(s0))
    assert s_same == int(s0) and np.array_equal(same, K0)


def test_prepare_kernel_serves_the_golden_bin2x2_case(gold, ims):
    got, s = ims.prepare_kernel(gold["e_K0"], int(gold["e_oversamp0"]), bin2x2=True)
    p = _pars(gold, "e")
    assert s == p["s"] and got.shape[1] == p["ax"]
    assert np.abs(got.astype(np.float64) - gold["e_K"]).max() <= 16 * 1.125**2 * (F32 / 2) * np.abs(gold["e_K0"]).max()
    with pytest.raises(ValueError):
        ims.prepare_kernel(gold["e_K0"], 5, bin2x2=True)  # 24 is not a multiple of 10
    with pytest.raises(ValueError):
        ims.prepare_kernel(gold["d_K"], 5, bin2x2=True)  # odd oversamp


def test_band_plan_counts_bytes_and_covers_the_rows(ims):
    nside, ax, s, Nl = 4088, 512, 8, 4
    I_pad, first, A = ims.geometry(ax, s, nside)
    assert (I_pad, first, A) == (32, 4, 8 * (4088 + 64))
    assert ims.plan_bands(nside, ax, s, Nl, 64 << 30, canvas_on_device=True) == [(0, nside)]
    free = 2 << 30
    bands = ims.plan_bands(nside, ax, s, Nl, free, canvas_on_device=False)
    assert len(bands) > 1 and bands[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(bands, bands[1:])) and sum(n for _, n in bands) == nside
    assert all(y0 % ims.TILE_ROWS == 0 for y0, _ in bands)
    for y0, ny in bands:
        lo, hi = ims.band_rows(y0, ny, ax, s, first)
        assert 0 <= lo < hi <= A and hi - lo == s * (ny - 1) + ax
        assert 4 * A * (hi - lo) + 4 * Nl * A + 256 <= ims.FILL * free
    # one more tile of rows would not fit
    rows = bands[0][1] + ims.TILE_ROWS
    assert 4 * A * (s * (rows - 1) + ax) + 4 * Nl * A + 256 > ims.FILL * free
    with pytest.raises(MemoryError):
        ims.plan_bands(nside, ax, s, Nl, 64 << 20, canvas_on_device=False)


@pytest.mark.parametrize("name", ["imcom_imsub_sizes", "imcom_imsub_prepare_kernel_f32", "imcom_imsub_canvas_add_f32", "imcom_imsub_convolve_subtract_f32"])
def test_entries_are_declared_with_their_reference_lines(name):
    txt = open(os.path.join(ROOT, "include", "imcom_hip.h")).read()
    assert name in txt and "imsubtract.py:689-707" in txt and "imsubtract.py:665-682" in txt
