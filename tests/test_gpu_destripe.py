"""Destriping on the device (pyimcom_amd.destripe, csrc/destripe.hip) against the reference's float64 run in tests/golden/destripe*.npz.
The bound of every quantity is the reference's own distance from that run (its float32 run, stored per quantity by
tests/golden/make_golden_destripe.py); psi, rounded once to float32 on store, has a floor of four float32 ulps of its maximum."""

import os

import numpy as np
import pytest

from tests import destripe_reference as dr
from tests.test_destripe_host import GOLDEN, load_case

pytestmark = pytest.mark.gpu
ULP32 = 2.0 ** -23


def engine_for(z, coords, order=None, lattice=None, **kw):
    from pyimcom_amd import destripe

    nside = int(z["nside"])
    eng = destripe.DestripeEngine(nside, nside, amp_cols=int(z["amp_cols"]) or None, col_boundary_const=float(z["col_boundary_const"]), **kw)
    for k in range(int(z["n_sca"])):
        eng.add_sca(z["image"][k], z["mask"][k], z["g_eff"][k])
    keys = sorted(coords) if order is None else order
    for a, b in keys:
        if lattice is None:
            eng.set_pair(a, b, x=coords[(a, b)][0], y=coords[(a, b)][1])
        else:
            eng.set_pair(a, b, lattice=lattice[(a, b)])
    return eng


def lattice_of(coef, nside, L=17):
    from pyimcom_amd import destripe

    nodes, _ = destripe.lattice_nodes(nside, L)
    u = nodes / nside - 0.5
    mono = [(i, j) for i in range(4) for j in range(4 - i)]
    return {k: np.stack([sum(c * np.outer(u ** j, u ** i) for c, (i, j) in zip(cf[p], mono)) for p in range(2)]) for k, cf in coef.items()}


@pytest.mark.parametrize("path", GOLDEN, ids=["rows", "amp_cols"])
def test_cost_and_gradient_against_the_float64_run(path):
    z, mos, coords, _, models = load_case(path)
    eng = engine_for(z, coords)
    d = np.abs(eng.N_eff.cpu().numpy() - z["neff"]).max()
    print(f"{os.path.basename(path)} N_eff: device {d:.3g}, reference {float(z['neff_ref_err']):.3g}")
    assert d <= float(z["neff_ref_err"])
    for name, thresh in models:
        eps, psi = eng.cost(z["params"], name, thresh)
        r = eng.residual(psi, name, thresh, extrareturn=True)
        tot = float(np.sum(z[f"{name}_eps"]))
        ref_eps = float(np.sum(np.abs(z[f"{name}_eps_ref_err"])))
        got = {"eps": abs(eps - tot), "psi": np.abs(psi.cpu().numpy() - z[f"{name}_psi"]).max()}
        bound = {"eps": ref_eps, "psi": max(float(z[f"{name}_psi_ref_err"]), 4 * ULP32 * np.abs(z[f"{name}_psi"]).max())}
        for got_r, q in zip(r, ("resids", "resids1", "resids2")):
            got[q] = np.abs(got_r - z[f"{name}_{q}"]).max()
            bound[q] = float(z[f"{name}_{q}_ref_err"])
        for q in got:
            print(f"{os.path.basename(path)} {name} {q}: device {got[q]:.3g} from the float64 run, the reference's float32 run {bound[q]:.3g}")
        for q in got:
            assert got[q] <= bound[q], (name, q, got[q], bound[q])


def _simple(kind, n=100):
    y, x = np.indices((n, n)).astype(np.float64)
    if kind == "gradient":
        return x + y
    if kind == "constant":
        return np.full((n, n), 13.0)
    if kind == "gaussian_peak":
        return np.exp(-((x - 30) ** 2 + (y - 30) ** 2) / (2 * 5.0 ** 2))
    return np.random.default_rng(13).random((n, n))


def test_the_references_assertions_on_the_two_routines():
    """tests/pyimcom/test_imdestripe.py 173-288 of the reference, with its thresholds, on the device routines."""
    from pyimcom_amd import destripe

    n = 100
    y, x = np.indices((n, n)).astype(np.float64)
    ones = np.ones((n, n))
    interior = np.ones((n, n), dtype=bool)
    interior[-1, :] = interior[:, -1] = False
    img = _simple("gradient")
    out = destripe.interpolate_bilinear(img, ones, x, y).cpu().numpy()
    assert np.allclose(out[interior], img[interior], atol=1e-8) and not out[~interior].any()
    out = destripe.transpose_bilinear(img, x, y, (n, n)).cpu().numpy()
    assert np.allclose(out[interior], img[interior]) and not out[~interior].any()
    xo, yo = x + 10.3, y + 5.6  # an offset map
    out = destripe.interpolate_bilinear(_simple("constant"), ones, xo, yo).cpu().numpy()
    valid = out != 0.0
    assert valid.sum() > 5000 and np.allclose(out[valid], 13.0)
    out = destripe.interpolate_bilinear(_simple("gaussian_peak"), ones, x - 6.0, y - 8.0).cpu().numpy()
    py, px = np.unravel_index(np.argmax(out), out.shape)
    assert 8 <= np.hypot(px - 30, py - 30) <= 16 and out.max() > 0.5
    a, b = _simple("random"), np.random.default_rng(14).random((n, n))
    lhs = np.sum(destripe.interpolate_bilinear(b, ones, xo, yo).cpu().numpy() * a)
    rhs = np.sum(b * destripe.transpose_bilinear(a, xo, yo, (n, n)).cpu().numpy())
    rel = abs(lhs - rhs) / (abs(lhs) + 1e-10)
    print("adjoint identity:", rel)
    assert rel < 1e-6


def test_gradient_is_the_derivative_of_the_cost():
    """residual against a central difference of cost in 20 seeded parameters (quadratic model, amp_cols and the penalty on).  The
    reference's gradient is not the exact derivative (N_eff != 0 against N_eff > N_eff_min, the penalty has no term in
    residual_function), so the mismatch itself says little; what is held is that the device's mismatch is the restatement's, pick by
    pick: both store psi as float32, so they may differ by the rounding of the two cost values (2^-40 of the cost over the step, four
    orders above float64's) plus the reference's own float32 distance of resids (golden file).  The issue's margin -- ten times the
    restatement's worst mismatch -- is asserted too."""
    z, mos, coords, _, _ = load_case(GOLDEN[1])
    mos.psi_dtype = np.float32
    eng = engine_for(z, coords)
    rng = np.random.default_rng(20)
    params = z["params"]
    picks = [(int(rng.integers(params.shape[0])), int(rng.integers(params.shape[1]))) for _ in range(18)] + [(0, params.shape[1] - 1), (2, params.shape[1] - 2)]
    h = 0.5

    def check(cost, residual):
        e0, psi = cost(params)
        g = residual(psi)
        errs = []
        for i, j in picks:
            pp, pm = params.copy(), params.copy()
            pp[i, j] += h
            pm[i, j] -= h
            errs.append((cost(pp)[0] - cost(pm)[0]) / (2 * h) - g[i, j])
        return np.asarray(errs), e0

    e_ref, cost0 = check(lambda p: mos.cost(p, "quadratic"), lambda psi: mos.residual(psi, "quadratic"))
    e_dev, _ = check(lambda p: eng.cost(p, "quadratic"), lambda psi: eng.residual(psi, "quadratic"))
    bound = 2.0 ** -40 * abs(cost0) / h + float(z["quadratic_resids_ref_err"])
    print(f"finite difference: worst mismatch device {np.abs(e_dev).max():.3g}, restatement {np.abs(e_ref).max():.3g}; "
          f"device against restatement per pick {np.abs(e_dev - e_ref).max():.3g}, bound {bound:.3g}")
    assert np.abs(e_dev - e_ref).max() <= bound
    assert np.abs(e_dev).max() <= 10 * np.abs(e_ref).max()


def test_same_bits_from_run_to_run_and_for_every_order_of_registration():
    z, _, coords, _, models = load_case(GOLDEN[1])
    runs = []
    for order in (None, None, sorted(coords, reverse=True)):
        eng = engine_for(z, coords, order=order)
        eps, psi = eng.cost(z["params"], "huber_loss", 4.0)
        runs.append((eps, psi.cpu().numpy(), eng.residual(psi, "huber_loss", 4.0)))
    for other in runs[1:]:
        assert other[0] == runs[0][0] and np.array_equal(other[1], runs[0][1]) and np.array_equal(other[2], runs[0][2])


@pytest.mark.parametrize("path", GOLDEN, ids=["rows", "amp_cols"])
def test_lattice_positions_give_what_the_full_arrays_give(path):
    """On polynomial maps the lattice reproduces the positions to 1e-10 pixels (the bound of test_sampling_positions_from_a_lattice).  A
    bilinear weight moves by at most 2 delta for positions delta apart, so N_eff moves by at most 2 delta per neighbour and a bin of the
    gradient by at most 2 delta times the sum of |g g_b| over the pixels of the pairs that feed it."""
    z, _, coords, coef, _ = load_case(path)
    nside, n_sca, delta = int(z["nside"]), int(z["n_sca"]), 1e-10
    full = engine_for(z, coords)
    lat = engine_for(z, coords, lattice=lattice_of(coef, nside))
    nf, nl = full.N_eff.cpu().numpy(), lat.N_eff.cpu().numpy()
    print("N_eff, lattice against full arrays:", np.abs(nf - nl).max())
    assert np.abs(nf - nl).max() <= 2 * delta * (n_sca - 1)
    eps, psi = full.cost(z["params"], "quadratic")
    rf, rl = full.residual(psi, "quadratic"), lat.residual(psi, "quadratic")
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(nf != 0, 2 * psi.cpu().numpy() / (z["g_eff"].astype(np.float64) * nf), 0)
    bound = 2 * delta * np.abs(g).sum(axis=(1, 2)).max() * (n_sca - 1) * float(z["g_eff"].max()) + 2.0 ** -40 * np.abs(rf).max()
    print("resids, lattice against full arrays:", np.abs(rf - rl).max(), "bound", bound)
    assert np.abs(rf - rl).max() <= bound
    eps_l, psi_l = lat.cost(z["params"], "quadratic")
    assert np.abs(psi_l.cpu().numpy() - psi.cpu().numpy()).max() <= 4 * ULP32 * np.abs(z["quadratic_psi"]).max()


def test_bound_functions_serve_the_references_signatures():
    """engine.bind: cost_function / residual_function with the reference's arguments and return types give what cost / residual give."""
    import types

    z, _, coords, _, _ = load_case(GOLDEN[0])
    eng = engine_for(z, coords)
    mod = eng.bind(types.SimpleNamespace())
    n_sca = int(z["n_sca"])
    scalist = [f"H158_{670 + k}_{k + 1}" for k in range(n_sca)]
    nb = {a: [b for b in range(n_sca) if b != a] for a in range(n_sca)}
    p = types.SimpleNamespace(params=z["params"].copy())
    f, fp = types.SimpleNamespace(__name__="huber_loss"), types.SimpleNamespace(__name__="huber_prime")
    eps, psi = mod.cost_function(p, f, 4.0, 8, scalist, nb, None)
    assert isinstance(psi, np.ndarray) and psi.dtype == np.float32 and psi.shape == (n_sca, 64, 64)
    res = mod.residual_function(psi, fp, scalist, [None] * n_sca, nb, 4.0, 8, None)
    e2, psi2 = eng.cost(z["params"], "huber_loss", 4.0)
    assert eps == e2 and np.array_equal(psi, psi2.cpu().numpy()) and np.array_equal(res, eng.residual(psi2, "huber_loss", 4.0))
    r, r1, r2 = mod.residual_function(psi.copy(), fp, scalist, [None] * n_sca, nb, 4.0, 8, None, extrareturn=True)
    assert np.array_equal(r, res) and np.array_equal(r, r2 + r1)
    with pytest.raises(ValueError):
        mod.cost_function(p, f, 4.0, 8, scalist, {0: [1]}, None)


def test_the_references_optimiser_on_top():
    """linear_search_quadratic and two iterations of conjugate_gradient over engine.bind.  The reference's program text is not in this
    tree; tests/golden/destripe_cg.npz holds the parameter vectors its optimiser evaluated and what it got back when the generator ran
    it (float64: the exact run; its float32 run's distance per call).  The recorded points are replayed through the bound functions in
    the recorded call order (destripe_reference.replay_line_searches, pinned to the record on the host): psi handed back as the array
    cost_function returned, the probe's psi dropped, parameters arriving through an object's ``params``.  Every eps, every resids and the
    points the line searches settle on, formed again from the device's gradients, are within the reference's own distance from the exact
    run."""
    import types

    zc = np.load(os.path.join(os.path.dirname(GOLDEN[0]), "destripe_cg.npz"))
    z, _, coords, _, _ = load_case(os.path.join(os.path.dirname(GOLDEN[0]), str(zc["source"])))
    eng = engine_for(z, coords)
    mod = eng.bind(types.SimpleNamespace())
    uploads = []
    resid = eng.residual
    eng.residual = lambda psi, *a, **k: (uploads.append(isinstance(psi, np.ndarray)), resid(psi, *a, **k))[1]
    n_sca = int(z["n_sca"])
    nb = {a: [b for b in range(n_sca) if b != a] for a in range(n_sca)}
    f, fp = types.SimpleNamespace(__name__="quadratic"), types.SimpleNamespace(__name__="quad_prime")
    got = dr.replay_line_searches(mod.cost_function, mod.residual_function, zc["params"], f, fp, [f"H158_{670 + k}_{k + 1}" for k in range(n_sca)], nb)
    assert len(got["eps"]) == len(zc["eps"]) and len(got["resids"]) == len(zc["resids"])
    assert uploads == [False] * len(zc["resids"])  # the device copy of the psi handed out was used every time
    d_eps = np.abs(np.asarray(got["eps"]) - zc["eps"])
    d_res = np.abs(np.stack(got["resids"]) - zc["resids"]).reshape(len(zc["resids"]), -1).max(axis=1)
    d_set = np.asarray([np.abs(x - zc["params"][2 * k + 2]).max() for k, x in enumerate(got["settled"])])
    print("optimiser on top: eps per call, device", d_eps, "reference", zc["eps_ref_err"])
    print("optimiser on top: resids per call, device", d_res, "reference", zc["resids_ref_err"])
    print("optimiser on top: points settled on, device", d_set, "reference", zc["params_ref_err"][2::2])
    assert (d_eps <= zc["eps_ref_err"]).all() and (d_res <= zc["resids_ref_err"]).all() and (d_set <= zc["params_ref_err"][2::2]).all()
    assert d_set[-1] <= float(zc["final_ref_err"][0])


def test_against_furry_parakeet_when_it_is_installed():
    """The two C routines themselves, for the first user who has the library: the device forward and transpose on the golden inputs."""
    fp = pytest.importorskip("furry_parakeet.pyimcom_interface")
    from pyimcom_amd import destripe

    z, _, coords, _, _ = load_case(GOLDEN[0])
    n = int(z["nside"])
    x, y = coords[(0, 1)]
    cc = np.column_stack((y.ravel(), x.ravel()))
    img, g = z["image"][1].astype(np.float64), z["g_eff"][1].astype(np.float64)
    img[np.isnan(img)] = 0
    want = np.zeros((n, n))
    fp.bilinear_interpolation(img, g, cc, want)
    assert np.abs(destripe.interpolate_bilinear(img, g, x, y).cpu().numpy() - want).max() <= 1e-12 * np.abs(want).max()
    want = np.zeros((n, n))
    fp.bilinear_transpose(img, cc, want)
    assert np.abs(destripe.transpose_bilinear(img, x, y, (n, n)).cpu().numpy() - want).max() <= 1e-9 * np.abs(want).max()
