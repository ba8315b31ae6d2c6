"""Host side of the destripe set-up made from WCSs (seam 21; no GPU): the registration rules of formed pairs, the byte plan, and the numpy
restatement of the effective gain (tests/destripe_setup_reference.py) pinned with ``==`` to the reference's own statements run over the same
float64 chain (tests/golden/destripe_setup.npz, tests/golden/make_golden_destripe_setup.py)."""

import json
import os

import numpy as np
import pytest

from tests import destripe_setup_reference as S
from tests.conftest import ROOT

G = np.load(os.path.join(ROOT, "tests", "golden", "destripe_setup.npz"))
CASES = {c["name"]: c for c in json.loads(str(G["meta"]))["cases"]}
WZ = np.load(os.path.join(ROOT, "tests", "golden", "wcs.npz"))


def table_of(case):
    return (WZ[f"table_{case['table']}"], float(WZ["table_ends"][0]), float(WZ["table_ends"][1])) if case["table"] else None


def small_engine(nside=64, n=3):
    from pyimcom_amd import destripe
    from pyimcom_amd import wcs as W

    h = dict(CASES["stg"]["header"])
    ws = []
    for k in range(n):
        hk = dict(h)
        hk["CRVAL1"] = h["CRVAL1"] + 0.0006 * k
        ws.append(W.DeviceWCS.from_header(hk, array_shape=(nside, nside)))
    eng = destripe.DestripeEngine(nside, nside)
    img = np.zeros((nside, nside), dtype=np.float32)
    for _ in range(n):
        eng.add_sca(img, img > -1, img + 1)
    return eng, ws, img


def test_formed_pairs_are_registered_from_two_wcs_only():
    eng, ws, img = small_engine()
    eng.set_pair(0, 1, wcs=(ws[0], ws[1]), keep_positions=False)  # (a TypeError before seam 21)
    eng.set_pair(1, 0, wcs=(ws[1], ws[0]), keep_positions=False)
    assert eng.neighbors() == {0: [1], 1: [0], 2: []} and eng.n_pairs == 2
    with pytest.raises(ValueError):
        eng.set_pair(0, 2, x=img, y=img, keep_positions=False)
    with pytest.raises(ValueError):
        eng.set_pair(0, 2, lattice=np.zeros((2, 17, 17)), keep_positions=False)
    with pytest.raises(ValueError):
        eng.set_pair(0, 2, keep_positions=False)
    with pytest.raises(ValueError):  # an SCA has one descriptor in all its formed pairs
        eng.set_pair(0, 2, wcs=(ws[1], ws[2]), keep_positions=False)
    eng.set_pair(0, 2, wcs=(ws[0], ws[2]), keep_positions=False)
    eng.set_pair(2, 0, wcs=(ws[2], ws[0]))  # the stored kind beside them
    assert eng.neighbors() == {0: [1, 2], 1: [0], 2: [0]}


def test_add_sca_takes_a_wcs_in_place_of_the_gain():
    eng, ws, img = small_engine(n=1)
    with pytest.raises(ValueError):
        eng.add_sca(img, img > -1)
    assert eng.add_sca(img, img > -1, wcs=ws[0]) == 1 and eng.add_sca(img, img > -1, img + 1, wcs=ws[0]) == 2
    from pyimcom_amd import wcs as W

    with pytest.raises(ValueError):
        eng.add_sca(img, img > -1, wcs=W.DeviceWCS.from_header(CASES["stg"]["header"], array_shape=(32, 32)))
    with pytest.raises(ValueError):  # SCA 0 came without a WCS
        eng.set_pairs_from_wcs()


def test_byte_plan_of_formed_pairs():
    from pyimcom_amd import destripe

    size = destripe.formed_pair_bytes(4088)
    assert 0 < size <= 1024  # nothing of the grid's size
    for k in (0, 1, 7):
        plan = destripe.memory_plan(4, 4088, 4088, 511, n_full=2, n_lattice=0, L=0, max_np=3, n_wcs=k)
        assert plan["pairs_wcs"] == k * size and plan["pairs_full"] == 2 * 16 * 4088 * 4088
        assert plan["total"] == sum(v for key, v in plan.items() if key not in ("nbins", "per_sca", "total"))
    eng, ws, _ = small_engine()
    assert eng.plan()["pairs_wcs"] == 0 and eng.plan()["wcs"] == 0
    for a, b in ((0, 1), (1, 0), (1, 2), (2, 1)):
        eng.set_pair(a, b, wcs=(ws[a], ws[b]), keep_positions=False)
    plan = eng.plan()
    assert plan["pairs_full"] == 0 and plan["pairs_lattice"] == 0 and plan["pairs_wcs"] == 4 * size
    assert plan["wcs"] == 3 * 130 * 8  # the descriptor table; these WCSs have no error table


def test_error_tables_are_counted_once_a_wcs():
    from pyimcom_amd import destripe
    from pyimcom_amd import wcs as W

    c = CASES["tab32_n3"]
    n = c["nside"]
    w = [W.DeviceWCS.from_header(c["header"], array_shape=(n, n), table=table_of(c), niter=3), W.DeviceWCS.from_header(c["header"], array_shape=(n, n)),
         W.DeviceWCS.from_header(c["header"], array_shape=(n, n))]
    eng = destripe.DestripeEngine(n, n)
    img = np.zeros((n, n), dtype=np.float32)
    for k in range(3):
        eng.add_sca(img, img > -1, img + 1)
    for a, b in ((0, 1), (1, 0), (0, 2), (2, 0)):
        eng.set_pair(a, b, wcs=(w[a], w[b]), keep_positions=False)
    assert eng.plan()["wcs"] == 3 * 130 * 8 + 2 * (n + 2) ** 2 * 4  # one float32 table, whatever the number of its pairs


def test_three_hundred_scas_fit_formed_and_not_stored():
    """The capacity the seam is about: 4088^2, 300 SCAs, 8 neighbours each, against FILL = 0.9 of 288 GB."""
    from pyimcom_amd import destripe

    room = 0.9 * 288e9
    formed = destripe.memory_plan(300, 4088, 4088, 511, n_full=0, n_lattice=0, L=0, max_np=8, n_wcs=2400, gain_setup=True)
    stored = destripe.memory_plan(300, 4088, 4088, 511, n_full=2400, n_lattice=0, L=0, max_np=8)
    assert formed["total"] < room < stored["total"], (formed["total"], stored["total"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_is_the_reference_run_bit_for_bit(name):
    c = CASES[name]
    desc = G[f"{name}_desc"]
    g64 = S.np_effective_gain(desc, table_of(c), c["nside"])
    assert g64.dtype == np.float64 and np.array_equal(g64, G[f"{name}_g64"])
    g32 = S.np_effective_gain(desc, table_of(c), c["nside"], np.float32)
    assert g32.dtype == np.float32 and np.array_equal(g32, G[f"{name}_g32"])
    assert np.max(np.abs(g64 - G[f"{name}_exact"])) == float(G[f"{name}_ref_err"][0])


def test_fixture_shows_the_transposition():
    """On the strongly distorted case the gain read WITHOUT the reference's transposition of its determinants is far from the fixture: the
    fixture decides the quirk (seam 8)."""
    name = "sip_asym"
    c = CASES[name]
    exact, g64 = G[f"{name}_exact"], G[f"{name}_g64"]
    _, dec = S.np_frame(G[f"{name}_desc"], None, c["nside"])
    cosd = np.cos(np.deg2rad(dec[1:-1, 1:-1]))
    untransposed = 1 / ((1 / (exact * cosd)).T * cosd)
    assert np.max(np.abs(g64 - exact)) < 1e-8 * g64.max() and np.max(np.abs(g64 - untransposed)) > 0.1 * g64.max()


def test_neighbour_rule():
    ov = np.array([[1.0, 0.3, 0.05], [0.3, 1.0, 0.1], [0.05, 0.1, 1.0]], dtype=np.float32)
    assert S.neighbors_of(ov, 0.1) == {0: [1], 1: [0, 2], 2: [1]}
    assert S.neighbors_of(ov, 0.2) == {0: [1], 1: [0], 2: []}
