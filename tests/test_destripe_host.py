"""Host side of the destriping seam (no GPU): the float64 restatement tests/destripe_reference.py is pinned bit for bit to the
reference's float64 run in tests/golden/destripe*.npz (tests/golden/make_golden_destripe.py), and the Python layer's host logic:
argument checks, the refusals, ``bind``, the byte plan, the lattice weights."""

import os
import types

import numpy as np
import pytest

from tests import destripe_reference as dr
from tests.conftest import ROOT

GOLDEN = [os.path.join(ROOT, "tests", "golden", f) for f in ("destripe.npz", "destripe_amp.npz")]


def load_case(path):
    z = np.load(path)
    nside, n_sca = int(z["nside"]), int(z["n_sca"])
    coef = {tuple(int(v) for v in k): c for k, c in zip(z["pairs"], z["coef"])}
    coords = {k: dr.poly_coords(c, nside) for k, c in coef.items()}
    mos = dr.Mosaic(z["image"], z["mask"], z["g_eff"], coords, amp_cols=int(z["amp_cols"]), col_boundary_const=float(z["col_boundary_const"]))
    models = [(str(m), None if np.isnan(t) else float(t)) for m, t in zip(z["models"], z["thresh"])]
    return z, mos, coords, coef, models


@pytest.mark.parametrize("path", GOLDEN, ids=["rows", "amp_cols"])
def test_restatement_is_the_float64_run_bit_for_bit(path):
    z, mos, _, _, models = load_case(path)
    assert np.array_equal(mos.neff, z["neff"])
    for name, thresh in models:
        eps, psi = mos.cost(z["params"], name, thresh)
        assert np.array_equal(psi, z[f"{name}_psi"]), name
        tot = 0
        for e in z[f"{name}_eps"]:
            tot += e
        assert eps == tot, (name, eps, tot)
        r, r1, r2 = mos.residual(psi, name, thresh, extrareturn=True)
        for got, q in ((r, "resids"), (r1, "resids1"), (r2, "resids2")):
            assert np.array_equal(got, z[f"{name}_{q}"]), (name, q, np.abs(got - z[f"{name}_{q}"]).max())


def test_generator_inputs_stay_clear_of_the_cell_edge():
    for path in GOLDEN:
        z, _, coords, _, _ = load_case(path)
        n = int(z["nside"])
        for x, y in coords.values():
            for v in (x, y):
                assert min(np.abs(v).min(), np.abs(v - (n - 1)).min()) > 1e-6


def test_cell_rule_of_the_stand_in():
    """What the reference's tests state of the C routine (test_imdestripe.py 173-189, 240-256): identity map, interior equal, last row
    and column zero -- forward and transpose.  This exercises tests/destripe_reference.py alone: it pins the assumption the golden files
    rest on, not the feature, and passes without the package's destriping code."""
    n = 20
    y, x = np.mgrid[:n, :n].astype(np.float64)
    img = x + 2 * y + 1
    coords = np.column_stack((y.ravel(), x.ravel()))
    out = np.zeros((n, n))
    dr.bilinear_interpolation(img, np.ones((n, n)), coords, out)
    assert np.array_equal(out[:-1, :-1], img[:-1, :-1]) and not out[-1].any() and not out[:, -1].any()
    out = np.zeros((n, n))
    dr.bilinear_transpose(img, coords, out)
    assert np.array_equal(out[:-1, :-1], img[:-1, :-1]) and not out[-1].any() and not out[:, -1].any()


def test_refusals_and_argument_checks():
    from pyimcom_amd import destripe
    from pyimcom_amd._lib import ImcomError

    with pytest.raises(ImcomError) as e:
        destripe.DestripeEngine(64, 64, ds_model="linear")
    assert e.value.status == -4
    with pytest.raises(ImcomError) as e:
        destripe.DestripeEngine(64, 64, amp_cols=24)
    assert e.value.status == -4 and "amp_cols" in str(e.value)
    with pytest.raises(ImcomError) as e:
        destripe.DestripeEngine(64, 32)
    assert e.value.status == -4
    with pytest.raises(ImcomError) as e:
        destripe.DestripeEngine(64, 64, amp_cols=32, col_boundary_const=1.0)
    assert e.value.status == -4
    eng = destripe.DestripeEngine(64, 64, amp_cols=16)
    assert eng.nbins == 68 and eng.n_col_blocks == 4
    img = np.zeros((64, 64), dtype=np.float32)
    with pytest.raises(ValueError):
        eng.add_sca(img[:32], img, img)
    assert eng.add_sca(img, img > -1, img + 1) == 0 and eng.add_sca(img, img > -1, img + 1) == 1
    with pytest.raises(ValueError):
        eng.set_pair(0, 0, x=img, y=img)
    with pytest.raises(ValueError):
        eng.set_pair(0, 2, x=img, y=img)
    with pytest.raises(ValueError):
        eng.set_pair(0, 1, x=img)
    with pytest.raises(ImcomError) as e:
        eng.set_pair(0, 1, lattice=np.zeros((2, 35, 35)))
    assert e.value.status == -4
    with pytest.raises(ValueError):
        eng.set_pair(0, 1, lattice=np.zeros((2, 17, 16)), L=17)
    eng.set_pair(1, 0, x=img, y=img)
    eng.set_pair(0, 1, lattice=np.zeros((2, 17, 17)))
    assert eng.neighbors() == {0: [1], 1: [0]}
    with pytest.raises(ValueError):
        destripe.model_name(np.sin)
    assert destripe.model_name(types.SimpleNamespace(__name__="huber_prime")) == "huber_loss"


def test_byte_plan_is_exact():
    from pyimcom_amd import destripe

    eng = destripe.DestripeEngine(4088, 4088, amp_cols=511)
    px = 4088 * 4088
    plan = destripe.memory_plan(4, 4088, 4088, 511, n_full=2, n_lattice=3, L=17, max_np=2)
    assert plan["per_sca"] == px * 21 and plan["scas"] == 4 * px * 21
    assert plan["pairs_full"] == 2 * px * 16 and plan["pairs_lattice"] == 3 * 17 * 17 * 16 and plan["weights"] == 4088 * 17 * 8
    assert plan["nbins"] == 4088 + 8
    assert plan["total"] == plan["scas"] + plan["pairs_full"] + plan["pairs_lattice"] + plan["weights"] + plan["params_and_resids"] + plan["workspace"] + plan["psi_upload"]
    assert plan["psi_upload"] == 4 * px * 4  # a second psi stack may be live
    assert plan["workspace"] >= 4 * 4088 * 8 * 8  # the rows' shares of the column blocks
    assert eng.plan()["scas"] == px * 21 and eng.n_pairs == 0


def test_bind_replaces_the_two_functions():
    from pyimcom_amd import destripe

    eng = destripe.DestripeEngine(64, 64)
    mod = types.SimpleNamespace(cost_function=None, residual_function=None, conjugate_gradient="kept")
    assert eng.bind(mod) is mod
    assert mod.cost_function == eng.cost_function and mod.residual_function == eng.residual_function and mod.conjugate_gradient == "kept"


def test_lattice_weights_reproduce_polynomial_maps():
    """The bound of test_sampling_positions_from_a_lattice (1e-10 on maps with quadratic and cubic terms), on the host formula."""
    from pyimcom_amd import destripe

    n = 100
    nodes, W = destripe.lattice_nodes(n, 17)
    assert W.shape == (n, 17) and np.abs(W.sum(axis=1) - 1).max() < 1e-13
    coef = dr.synthetic_maps(3, n, 5)[(0, 1)]
    x, y = dr.poly_coords(coef, n)
    u, v = nodes / n - 0.5, nodes / n - 0.5
    for k, full in enumerate((x, y)):
        lat = sum(c * np.outer(v ** j, u ** i) for c, (i, j) in zip(coef[k], [(i, j) for i in range(4) for j in range(4 - i)]))
        assert np.abs(W @ lat @ W.T - full).max() < 1e-10


def test_replay_of_the_recorded_optimiser_run():
    """tests/golden/destripe_cg.npz: two iterations of the reference's conjugate_gradient with linear_search_quadratic, run by the
    generator with the reference's own functions (float64) and with the restatement bound in -- the two asserted equal there.  Replaying
    the recorded evaluation points over the restatement gives every eps and resids of the record bit for bit, and the points the line
    searches settled on, formed again from the gradients (destripe_reference.replay_line_searches), are the recorded ones up to the
    1e-12 the reference adds to its denominators."""
    import types

    zc = np.load(os.path.join(ROOT, "tests", "golden", "destripe_cg.npz"))
    z, mos, _, _, _ = load_case(os.path.join(ROOT, "tests", "golden", str(zc["source"])))
    f, fp = types.SimpleNamespace(__name__="quadratic"), types.SimpleNamespace(__name__="quad_prime")
    n_sca = int(z["n_sca"])
    nb = {a: [b for b in range(n_sca) if b != a] for a in range(n_sca)}
    got = dr.replay_line_searches(mos.cost_function, mos.residual_function, zc["params"], f, fp, [""] * n_sca, nb)
    assert np.array_equal(np.asarray(got["eps"]), zc["eps"]) and np.array_equal(np.stack(got["resids"]), zc["resids"])
    assert np.array_equal(zc["params"][4], zc["final"])
    for k, x in enumerate(got["settled"]):
        assert np.abs(x - zc["params"][2 * k + 2]).max() <= 1e-9 * np.abs(zc["params"][2 * k + 2]).max()
