"""The reference of the Eigen kernel's edge tests checked against the reference implementation's own recorded outputs and against
itself, before any GPU run: tests/eigen_reference.py."""

import numpy as np
import pytest

from tests import eigen_reference as er
from tests.test_oracle import indef_case

RTOL_MAP, ATOL_MAP = er.RTOL_MAP, er.ATOL_MAP


def _golden_cases(golden):
    """(tag, A, mB [m][n], C, kC, target, smax, recorded kappa / UC / Sigma [m]) of every multi-kappa Eigen record of the goldens."""
    la = golden("lakernel")
    out = []
    # (nodes, leakage target, sigma_max of the lakernel golden's records: EIG_CASES of tests/test_gpu_routines.py)
    for name, kC, target, smax in (("cos", np.array([1e-4, 1e-3, 1e-2]), 1e-4, 1.0), ("gau", np.array([1e-5, 1e-4, 1e-3]), 1e-6, 0.5)):
        A, mB, Cs = la[f"{name}_A"], la[f"{name}_mBhalf"], np.atleast_1d(la[f"{name}_C"])
        for j in range(mB.shape[0]):
            rec = [la[f"{name}_eigm_{q}"][j].ravel() for q in ("kappa", "UC", "Sigma")]
            out.append((f"{name}[{j}]", A, mB[j], float(Cs[j]), kC, target, smax, *rec))
    for name in ("repair", "gau", "chain"):
        g, A, mB, Cs, _ = indef_case(golden, name)
        for j in range(mB.shape[0]):
            rec = [g[f"{name}_eigm_{q}"][j].ravel() for q in ("kappa", "UC", "Sigma")]
            out.append((f"indef {name}[{j}]", A, mB[j], float(Cs[j]), g[f"{name}_eigm_kappaC"], float(g[f"{name}_uctarget"]),
                        float(g[f"{name}_sigmamax"]), *rec))
    return out


def test_replay_of_the_recorded_kappa_finds_the_reference_decisions(golden):
    """The reference's own kappa (float32, times C) decodes to a node at every pixel, and every decision on that path is the one the
    long-double sums give."""
    for tag, A, mB, C, kC, target, smax, kap, _, _ in _golden_cases(golden):
        lam, Q = np.linalg.eigh(A)
        ok, dev, ref, margin, _ = er.replay(lam, mB @ Q, C, kC[0] * C, kC[-1] * C, target, smax, 13, kap)
        assert ok.all(), tag
        assert np.array_equal(dev, ref), (tag, np.argwhere(dev != ref)[:4], margin[dev != ref][:4])


def test_maps_at_reproduces_the_recorded_maps(golden):
    for tag, A, mB, C, kC, _, _, kap, UC, Sg in _golden_cases(golden):
        ok, up = er.decode(kap, C, kC[0] * C, kC[-1] * C, 13)
        assert ok.all(), tag
        k = er.path(up, kC[0] * C, kC[-1] * C)[:, -1].astype(np.float64)
        _, Ur, Sr, scale = er.maps_at(A, mB, C, k)
        # (the indefinite goldens' forward error eps |A| / min |lam + kappa| is 3e-8 at worst: tests/test_gpu_eigen_indef.py)
        assert np.all(np.abs(UC - Ur) <= ATOL_MAP + RTOL_MAP * np.maximum(np.abs(Ur), scale)), (tag, np.abs(UC - Ur).max())
        assert np.allclose(Sg, Sr, rtol=RTOL_MAP, atol=ATOL_MAP), tag


def test_decoder_rejects_kappa_between_nodes():
    kmin, kmax, C, nbis = 3e-4, 3.0, 1.1, 13
    lnr = er.grid_step(kmin, kmax, nbis)
    mid = np.sqrt(kmin * kmax)
    j = np.array([-8191, -1, 1, 4097, 8191])
    on = er.quirk(mid * np.exp(j * lnr), C)
    ok, up = er.decode(on, C, kmin, kmax, nbis)
    assert ok.all()
    assert not up[0].any() and up[-1].all() and up[1].tolist() == [False] + [True] * 12 and up[2].tolist() == [True] + [False] * 12
    assert np.allclose(er.path(up, kmin, kmax)[:, -1].astype(np.float64), mid * np.exp(j * lnr), rtol=1e-12)
    half = er.quirk(mid * np.exp((j + 0.5) * lnr), C)
    assert not er.decode(half, C, kmin, kmax, nbis)[0].any()
    assert not er.decode(er.quirk(mid * np.exp(np.array([0.0, 2.0, 8193.0, -8193.0]) * lnr), C), C, kmin, kmax, nbis)[0].any()  # even / outside
    assert not er.decode(np.array([np.nan, 0.0, -1.0], np.float32), C, kmin, kmax, nbis)[0].any()
    assert er.decode(er.quirk(np.array([mid]), C), C, kmin, kmax, 0)[0].all()
    assert not er.decode(er.quirk(np.array([mid * np.exp(0.5 * er.grid_step(kmin, kmax, 0))]), C), C, kmin, kmax, 0)[0].any()


@pytest.mark.parametrize("name", list(er.SEARCH_CASES))
def test_sums_agree_with_maps_at_and_few_reference_decisions_are_within_the_bound(name):
    """On every committed case with decisions: the long-double eigen-sums that replay the decisions lie within the decision bound
    of maps_at at the final kappa of every pixel, and at most 2 % of the pixels hold a decision whose margin is below the bound
    anywhere on the reference's own path (so that statement (b) is not vacuous)."""
    case = er.SEARCH_CASES[name]()
    tied, total, _ = er.tied_pixels(case)
    assert tied <= er.MAX_TIED * total, (tied, total)
    for st, _ in er.distinct(case.stamps):
        if st.n == 0:
            continue
        lam, P = st.eig()
        kmin, kmax = case.ends(st)
        k, _ = er.bisect(lam, P, st.C, kmin, kmax, case.target, case.smax, case.nbis)
        S, udc, scale = er.sums(lam, P, st.C, k)
        _, Ur, Sr, scale_r = er.maps_at(st.A, st.mB, st.C, k)
        bound = er.dec_bound(st.n, er.cond_sym(lam, kmin), lam[0] + kmin <= 0)
        assert np.all(np.abs(udc.astype(np.float64) - Ur) <= bound * scale_r), (st.n, (np.abs(udc.astype(np.float64) - Ur) / scale_r).max() / bound)
        assert np.all(np.abs(S.astype(np.float64) - Sr) <= bound * Sr), (st.n, (np.abs(S.astype(np.float64) - Sr) / Sr).max() / bound)
        assert np.allclose(scale.astype(np.float64), scale_r, rtol=1e-6)


def test_search_cases_take_decisions_both_ways():
    """The size-edge search cases end strictly inside the bracket for most pixels: the ends of the bracket do not dominate."""
    for m in (63, 64, 65):
        for q in (0.3, 0.7):
            _, total, inside = er.tied_pixels(er.search_case(m, q))
            assert inside >= 0.85 * total, (m, q, inside, total)
    c = er.smax_case()
    alone = 0
    for st, _ in er.distinct(c.stamps):
        if st.n:
            lam, P = st.eig()
            kmin, kmax = c.ends(st)
            k, _ = er.bisect(lam, P, st.C, kmin, kmax, c.target, c.smax, c.nbis)
            alone += int(er.replay(lam, P, st.C, kmin, kmax, c.target, c.smax, c.nbis, er.quirk(k, st.C))[4].any(1).sum())
    assert alone >= 16 * c.m / 3


def test_lu_refined_solve_is_the_cholesky_one_where_both_apply_and_solves_indefinite_systems():
    from tests import la_reference as ref

    rng = np.random.default_rng(3)
    st, = er.systems((40,), 5, rng)
    X = ref.solve_refined(st.A, 1e-3, st.mB.T)
    Y = ref.solve_refined_lu(st.A, 1e-3, st.mB.T)
    assert np.abs(X - Y).max() <= 1e-15 * np.abs(X).max()
    w = np.concatenate([-rng.uniform(1, 2, 20), rng.uniform(1, 2, 21)])
    A, _ = ref.with_spectrum(w, rng)
    B = rng.standard_normal((41, 3))
    Z = ref.solve_refined_lu(A, 0.05, B)
    AL = A.astype(ref.LD)
    AL[np.diag_indices(41)] += ref.LD(0.05)
    assert np.abs(AL @ Z - B).max() <= 1e-17 * np.abs(Z).max()  # a long-double residual: far below float64's 1e-16
