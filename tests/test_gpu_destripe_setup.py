"""The destripe set-up made from WCSs on the device (seam 21): pair positions formed in the kernels of csrc/destripe.hip, the effective gain
(csrc/wcs.hip) and the neighbour table.

Formed pairs are held to the stored ones with ``==``: the kernels call the inline function that ``imcom_wcs_pix2pix`` stored its arrays
with, on the same integer pixel.  The gain is held to the 40-digit evaluation of the reference's statements within 10 times the
reference's own distance from it (tests/golden/destripe_setup.npz), the standing bound of seams 16 to 18."""

import os
import types

import numpy as np
import pytest

from tests import destripe_reference as dr
from tests import destripe_setup_reference as S
from tests import wcs_reference as R
from tests.conftest import ROOT
from tests.test_destripe_setup_host import CASES as GAIN_CASES
from tests.test_destripe_setup_host import G as GAIN
from tests.test_destripe_setup_host import table_of as gain_table_of

pytestmark = pytest.mark.gpu

WZ = np.load(os.path.join(ROOT, "tests", "golden", "wcs.npz"))
WCS_CASES = {c["name"]: c for c in __import__("json").loads(str(WZ["meta"]))["cases"]}
KINDS = {"sip_a": "small_a", "sip_b": "small_b", "sip_c": "small_d", "stg": "stg_m40", "tab": "tab32_n3"}
MODELS = (("quadratic", None), ("huber_loss", 4.0))


def make_wcs(kind, nside, dra=0.0, ddec=0.0):
    """A header of tests/golden/wcs.npz re-centred on an SCA of ``nside`` pixels at (150 + dra, 2.2 + ddec) degrees; ``tab``: with a float32
    error table made by ``wcs.error_table`` from a smooth map of a few hundredths of a pixel, niter = 3."""
    from pyimcom_amd import wcs as W

    h = dict(WCS_CASES[KINDS[kind]]["header"])
    h["CRPIX1"] = h["CRPIX2"] = (nside + 1) / 2
    h["CRVAL1"], h["CRVAL2"] = 150.0 + dra, 2.2 + ddec
    table = None
    if kind == "tab":
        y, x = np.mgrid[0:nside, 0:nside] / float(nside)
        m = np.stack((0.04 * np.sin(3.1 * x + 1.3 * y) + 0.01 * x * y, 0.03 * np.cos(2.2 * y - 0.7 * x) - 0.02 * y * y))
        table = W.error_table(m + 2e-3 * np.random.default_rng(77).standard_normal(m.shape), a=8, use_float32=True)
        assert table[0].dtype == np.float32
    return W.DeviceWCS.from_header(h, array_shape=(nside, nside), table=table, niter=3 if kind == "tab" else 0)


def scas_of(n_sca, nside, seed):
    rng = np.random.default_rng(seed)
    return [(rng.normal(100.0, 5.0, (nside, nside)).astype(np.float32), rng.random((nside, nside)) > 0.1, rng.uniform(0.9, 1.1, (nside, nside)).astype(np.float32))
            for _ in range(n_sca)]


def shifted(kinds, nside):
    """SCA k about 20 pixels from SCA k - 1."""
    return [make_wcs(kind, nside, 0.0006 * k, 0.0004 * k) for k, kind in enumerate(kinds)]


def evaluate(eng, params):
    """Everything the two functions return, for the two models, as host arrays."""
    out = {"N_eff": eng.N_eff.cpu().numpy()}
    for name, thresh in MODELS:
        eps, psi = eng.cost(params, name, thresh)
        r, r1, r2 = eng.residual(psi, name, thresh, extrareturn=True)
        out.update({f"{name}_eps": eps, f"{name}_psi": psi, f"{name}_resids": r, f"{name}_r1": r1, f"{name}_r2": r2, f"{name}_plain": eng.residual(psi, name, thresh)})
    return out


def assert_same_bits(got, want):
    import torch

    assert sorted(got) == sorted(want)
    for k in want:
        if k.endswith("_psi"):
            assert torch.equal(got[k], want[k]), k
        elif k.endswith("_eps"):
            assert got[k] == want[k], (k, got[k], want[k])
        else:
            assert np.array_equal(got[k], want[k]), (k, np.abs(got[k] - want[k]).max())


def all_pairs(n):
    return [(a, b) for a in range(n) for b in range(n) if a != b]


def engine(scas, ws, pairs, keep, nside, order=None, **kw):
    from pyimcom_amd.destripe import DestripeEngine

    eng = DestripeEngine(nside, nside, **kw)
    for s in scas:
        eng.add_sca(*s)
    for a, b in (order or pairs):
        eng.set_pair(a, b, wcs=(ws[a], ws[b]), keep_positions=keep)
    return eng


MOSAICS = {
    # nside, the SCAs' WCSs, engine options
    "64_sip_sip": (64, ("sip_a", "sip_b"), {}),
    "64_sip_stg": (64, ("sip_b", "stg"), {}),
    "64_tab_sip": (64, ("tab", "sip_a"), {}),  # the table on the target's side of (0, 1) and on the reference's side of (1, 0)
    "100_amp_cols": (100, ("sip_a", "tab", "sip_b"), {"amp_cols": 50, "col_boundary_const": 1.0}),  # not a multiple of the wave; penalty on
    "257_rows": (257, ("sip_b", "stg", "sip_a"), {}),  # a second pass of the column loop with one live lane
}


@pytest.mark.parametrize("name", sorted(MOSAICS))
def test_formed_pairs_give_the_bits_of_stored_pairs(name):
    nside, kinds, kw = MOSAICS[name]
    ws, scas = shifted(kinds, nside), scas_of(len(kinds), nside, 21)
    pairs = all_pairs(len(kinds))
    formed, stored = engine(scas, ws, pairs, False, nside, **kw), engine(scas, ws, pairs, True, nside, **kw)
    assert formed.plan()["pairs_full"] == 0 and formed.plan()["pairs_wcs"] > 0 and stored.plan()["pairs_wcs"] == 0
    assert formed.plan()["total"] < stored.plan()["total"]
    params = np.random.default_rng(5).normal(0.0, 1.0, (len(kinds), formed.nbins))
    want = evaluate(stored, params)
    assert want["N_eff"].max() > 0.5 and np.abs(want["quadratic_r2"]).max() > 0 and np.count_nonzero(want["quadratic_psi"].cpu().numpy()) > nside
    assert_same_bits(evaluate(formed, params), want)


def mixed_engine(scas, ws, nside, keep, order=None):
    """Four SCAs: (0, 1), (1, 0) from uploaded arrays, (0, 2), (2, 0) on a lattice (an affine map), the rest from WCSs (formed or stored)."""
    from pyimcom_amd import destripe
    from pyimcom_amd import wcs as W

    eng = destripe.DestripeEngine(nside, nside)
    for s in scas:
        eng.add_sca(*s)
    nodes, _ = destripe.lattice_nodes(nside, 5)
    for a, b in (order or all_pairs(4)):
        if {a, b} == {0, 1}:
            x, y, _ = W.map_sca2sca(ws[a], ws[b], pad=0)
            eng.set_pair(a, b, x=x, y=y)
        elif {a, b} == {0, 2}:
            sign = 1.0 if a == 0 else -1.0
            eng.set_pair(a, b, lattice=np.stack((np.tile(nodes + sign * 13.3, (5, 1)), np.tile((nodes - sign * 7.7)[:, None], (1, 5)))))
        else:
            eng.set_pair(a, b, wcs=(ws[a], ws[b]), keep_positions=keep)
    return eng


def test_mixed_sources_in_one_engine():
    nside = 64
    ws, scas = shifted(("sip_a", "sip_b", "stg", "tab"), nside), scas_of(4, nside, 22)
    formed, stored = mixed_engine(scas, ws, nside, False), mixed_engine(scas, ws, nside, True)
    p = formed.plan()
    assert p["pairs_full"] > 0 and p["pairs_lattice"] > 0 and p["pairs_wcs"] == 8 * formed_bytes() and stored.plan()["pairs_wcs"] == 0
    params = np.random.default_rng(6).normal(0.0, 1.0, (4, formed.nbins))
    want = evaluate(stored, params)
    assert_same_bits(evaluate(formed, params), want)
    # every source contributes: taking a pair of each kind away changes N_eff of its target
    for drop in ((0, 1), (0, 2), (0, 3)):
        less = mixed_engine(scas, ws, nside, False, order=[k for k in all_pairs(4) if k != drop])
        assert not np.array_equal(less.N_eff.cpu().numpy()[0], want["N_eff"][0]), drop


def formed_bytes():
    from pyimcom_amd import destripe

    return destripe.formed_pair_bytes(64)


def test_a_reference_on_the_far_side_of_the_sky_contributes_nothing():
    """The antipode case of tests/test_gpu_wcs.py: every position has no image.  The stored path holds NaN there; the formed one forms it."""
    from pyimcom_amd import wcs as W

    nside = 64
    ws = shifted(("sip_a", "sip_b"), nside)
    h = dict(WCS_CASES["small_a"]["header"])
    h["CRPIX1"] = h["CRPIX2"] = (nside + 1) / 2
    h["CRVAL1"], h["CRVAL2"] = 150.0 + 180.0, -2.2
    ws.append(W.DeviceWCS.from_header(h, array_shape=(nside, nside)))
    x, _, m = W.map_sca2sca(ws[0], ws[2], pad=0)
    assert np.isnan(x).all() and not m.any()
    scas = scas_of(3, nside, 23)
    pairs = all_pairs(3)
    formed, stored = engine(scas, ws, pairs, False, nside), engine(scas, ws, pairs, True, nside)
    without = engine(scas[:2], ws[:2], all_pairs(2), False, nside)
    params = np.random.default_rng(7).normal(0.0, 1.0, (3, nside))
    got, want, two = evaluate(formed, params), evaluate(stored, params), evaluate(without, params[:2])
    assert_same_bits(got, want)
    assert not got["N_eff"][2].any() and np.array_equal(got["N_eff"][:2], two["N_eff"])
    # (the gradients of the two mosaics are not compared: their fixed-point scale depends on the number of SCAs)
    assert np.array_equal(got["quadratic_psi"].cpu().numpy()[:2], two["quadratic_psi"].cpu().numpy()) and np.array_equal(got["quadratic_r2"][2], np.zeros(nside))


def test_formed_pairs_same_bits_from_run_to_run_and_for_every_order_of_registration():
    nside = 100
    ws, scas = shifted(("sip_a", "tab", "sip_b"), nside), scas_of(3, nside, 24)
    pairs = all_pairs(3)
    params = np.random.default_rng(8).normal(0.0, 1.0, (3, nside + 2))
    runs = [evaluate(engine(scas, ws, pairs, False, nside, order=order, amp_cols=50, col_boundary_const=1.0), params) for order in (None, None, pairs[::-1])]
    eng = engine(scas, ws, pairs, False, nside, amp_cols=50, col_boundary_const=1.0)
    runs.append(evaluate(eng, params))
    runs.append(evaluate(eng, params))  # the same engine again
    for other in runs[1:]:
        assert_same_bits(other, runs[0])


def test_c_abi_refuses_a_formed_pair_without_its_wcs_arguments():
    import torch

    from pyimcom_amd import _lib

    ctx = _lib.default_context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    n = 16
    mask = torch.ones((2, n, n), dtype=torch.uint8, device="cuda")
    neff = torch.zeros((2, n, n), dtype=torch.float64, device="cuda")
    pa, pb, nul = np.array([0], dtype=np.int32), np.array([1], dtype=np.int32), np.zeros(1, dtype=np.uint64)
    desc = torch.zeros((2, 130), dtype=torch.float64, device="cuda")
    rot = torch.zeros((1, 9), dtype=torch.float64, device="cuda")

    def call(*wcs):
        return _lib.lib.imcom_destripe_neff(ctx.handle, 2, n, 0, _lib.ptr(mask), 1, _lib.ptr(pa), _lib.ptr(pb), _lib.ptr(nul), _lib.ptr(nul), _lib.ptr(nul), None,
                                            _lib.ptr(neff), *wcs)

    assert call(None, None, None, None, None, None, None) == -1 and "WCS" in _lib.lib.imcom_last_error().decode()
    assert call(_lib.ptr(desc), None, None, None, None, None, None) == -1  # the rotation products are missing
    assert call(_lib.ptr(desc), _lib.ptr(nul), None, None, None, None, _lib.ptr(rot)) == -1  # the five table arrays come together
    # an all-zero descriptor table: every position is formed from a singular WCS and is NaN -- nothing is gathered, nothing faults
    assert call(_lib.ptr(desc), None, None, None, None, None, _lib.ptr(rot)) == 0
    torch.cuda.synchronize()
    assert not neff.any()
    bad = np.zeros(130)
    M = np.zeros(9)
    assert _lib.lib.imcom_destripe_pair_rotation(_lib.ptr(bad), _lib.ptr(bad), _lib.ptr(M)) == -1  # (a singular CD matrix)


# ---- the gain ---------------------------------------------------------------------------------------------------------------------------------

def gain_wcs(name):
    from pyimcom_amd import wcs as W

    c = GAIN_CASES[name]
    w = W.DeviceWCS.from_header(c["header"], array_shape=(c["nside"], c["nside"]), table=gain_table_of(c), niter=c["niter"])
    assert np.array_equal(w.descriptor, GAIN[f"{name}_desc"])
    return w, c["nside"]


@pytest.mark.parametrize("name", sorted(GAIN_CASES))
def test_effective_gain_against_the_fixture(name):
    from pyimcom_amd import destripe

    w, nside = gain_wcs(name)
    exact, ref_err = GAIN[f"{name}_exact"], float(GAIN[f"{name}_ref_err"][0])
    g64 = destripe.effective_gain(w, nside, dtype=np.float64)
    assert g64.shape == (nside, nside) and g64.dtype == np.float64
    err = np.abs(g64 - exact)
    print(f"{name}: |device float64 - 40-digit| at most {err.max():.3e}, the reference's own {ref_err:.3e}, ratio {err.max() / ref_err:.3f} (bound 10)")
    assert np.all(err <= 10 * ref_err)
    g32 = destripe.effective_gain(w, nside)
    assert g32.dtype == np.float32 and np.array_equal(g32, g64.astype(np.float32))
    want = GAIN[f"{name}_g32"]
    differ = g32 != want
    print(f"{name}: {np.count_nonzero(differ)} of {differ.size} float32 values differ from the reference's")
    # only where the two float64 values, both within the bound, round to different float32 numbers: then to adjacent ones
    assert np.array_equal(np.nextafter(g32[differ], want[differ]), want[differ])
    assert np.all(np.abs(GAIN[f"{name}_g64"][differ] - exact[differ]) <= 10 * ref_err) and np.all(err[differ] <= 10 * ref_err)
    dev = destripe.effective_gain(w, nside, device_out=True)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), g32)


def test_gain_made_at_upload_is_the_gain_handed_in():
    from pyimcom_amd import destripe

    nside = 64
    ws, scas = shifted(("sip_a", "tab"), nside), scas_of(2, nside, 25)
    made = [(s[0], s[1], None) for s in scas]
    given = [(s[0], s[1], destripe.effective_gain(w, nside)) for s, w in zip(scas, ws)]
    params = np.random.default_rng(9).normal(0.0, 1.0, (2, nside))
    runs = []
    for rows in (made, given):
        eng = destripe.DestripeEngine(nside, nside)
        for (im, ma, ge), w in zip(rows, ws):
            eng.add_sca(im, ma, ge, wcs=w)
        for a, b in all_pairs(2):
            eng.set_pair(a, b, wcs=(ws[a], ws[b]), keep_positions=False)
        runs.append(evaluate(eng, params))
    assert_same_bits(runs[0], runs[1])
    assert np.abs(runs[0]["quadratic_r2"]).max() > 0


# ---- the neighbours ---------------------------------------------------------------------------------------------------------------------------

def test_neighbours_from_the_wcss_of_five_small_chips():
    from pyimcom_amd import destripe
    from pyimcom_amd import wcs as W

    names = ["small_a", "small_b", "small_c", "small_d", "small_e"]
    ws = [W.DeviceWCS.from_header(WCS_CASES[n]["header"], array_shape=(250, 250)) for n in names]
    want = R.np_overlap_matrix([WZ[n + "_desc"] for n in names], 250, pad=2, subsamp=3)
    v = float(want[1, 0])
    assert 0 < v < 1
    img = np.zeros((250, 250), dtype=np.float32)
    seen = []
    for t in (0.9 * v, 1.1 * v):
        eng = destripe.DestripeEngine(250, 250)
        for w in ws:
            eng.add_sca(img, img > -1, img + 1, wcs=w)
        ov, nb = eng.set_pairs_from_wcs(overlap_thresh=t, subsamp=3, pad=2)
        assert ov.dtype == np.float32 and np.array_equal(ov, want)
        assert nb == S.neighbors_of(want, t) and eng.neighbors() == nb and eng.n_pairs == sum(len(x) for x in nb.values())
        assert eng.plan()["pairs_full"] == 0 and eng.plan()["pairs_wcs"] == eng.n_pairs * destripe.formed_pair_bytes(250)
        seen.append(nb)
    assert 1 in seen[0][0] and 1 not in seen[1][0] and seen[0][3] == [] and seen[0][4] == []


# ---- the optimiser on top ---------------------------------------------------------------------------------------------------------------------

def test_the_optimiser_on_formed_pairs_and_device_made_gain():
    """destripe_reference.replay_line_searches over the recorded parameter vectors of tests/golden/destripe_cg.npz, through an engine whose
    gain and pairs come from WCSs alone and through one that is handed the gain and keeps the positions: every eps, every resids and the
    points the line searches settle on are the same bits."""
    from pyimcom_amd import destripe
    from tests.test_destripe_host import load_case

    golden = os.path.join(ROOT, "tests", "golden")
    zc = np.load(os.path.join(golden, "destripe_cg.npz"))
    z, _, _, _, _ = load_case(os.path.join(golden, str(zc["source"])))
    nside, n_sca = int(z["nside"]), int(z["n_sca"])
    kinds = ("sip_a", "sip_b", "stg", "tab", "sip_c")
    ws = shifted([kinds[k % len(kinds)] for k in range(n_sca)], nside)
    nb = {a: [b for b in range(n_sca) if b != a] for a in range(n_sca)}
    f, fp = types.SimpleNamespace(__name__="quadratic"), types.SimpleNamespace(__name__="quad_prime")
    runs = []
    for from_wcs in (True, False):
        eng = destripe.DestripeEngine(nside, nside, amp_cols=int(z["amp_cols"]) or None, col_boundary_const=float(z["col_boundary_const"]))
        for k in range(n_sca):
            eng.add_sca(z["image"][k], z["mask"][k], None if from_wcs else destripe.effective_gain(ws[k], nside), wcs=ws[k])
        for a, b in all_pairs(n_sca):
            eng.set_pair(a, b, wcs=(ws[a], ws[b]), keep_positions=not from_wcs)
        mod = eng.bind(types.SimpleNamespace())
        runs.append(dr.replay_line_searches(mod.cost_function, mod.residual_function, zc["params"], f, fp, [""] * n_sca, nb))
    a, b = runs
    assert len(a["eps"]) == len(zc["eps"]) and a["eps"] == b["eps"]
    assert np.array_equal(np.stack(a["resids"]), np.stack(b["resids"])) and np.abs(np.stack(a["resids"])).max() > 0
    assert all(np.array_equal(x, y) for x, y in zip(a["settled"], b["settled"])) and len(a["settled"]) == len(b["settled"])
