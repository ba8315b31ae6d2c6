"""The reference of the coaddition epilogue's edge tests (tests/epilogue_reference.py) checked before any GPU run: against the
reference implementation's own recorded coaddition (tests/golden/coadd_stamp.npz), against numpy's float64 statement of the same
step (oracle.perform_coaddition) within the derived bounds, on the conditions its inputs promise, and on the comparator's
sensitivity to the index errors the GPU suite is there to find."""

import numpy as np
import pytest

from oracle import oracle as orc
from tests import epilogue_reference as ep

LD = ep.LD
BY_NAME = {c.name: c for c in ep.CASES}


def _oracle_f64(case, data):
    """oracle.perform_coaddition per stamp on the transposed views: once on the float32 T with the fade (the taper of T, in place),
    once in float64 on the tapered values (the sums), Neff's taper after it."""
    Tt, x, e = data
    batch, m = len(case.ns), case.m
    got = dict(T=[], outimage=np.zeros((batch, case.n_inframe, m), np.float32), Tsum_stamp=np.zeros((batch, case.n_expo)),
               Tsum_inpix=np.zeros((batch, m)), Neff=np.zeros((batch, m)))
    for s, ns in enumerate(case.ns):
        T = np.array(Tt[s, :ns, :m].T, order="C")[None]  # [1][m][ns] float32, a copy
        xs, es = x[s, :, :ns], e[s, :ns]
        with np.errstate(invalid="ignore", divide="ignore"):
            orc.perform_coaddition(T, xs, es, case.n_expo, case.n2f, case.n2, case.fade)
            img, st, inpix, neff = orc.perform_coaddition(T.astype(np.float64), xs.astype(np.float64), es, case.n_expo, case.n2f, case.n2, 0)
        neff = neff[0].copy()
        orc.trapezoid(neff, case.fade)
        got["T"].append(T[0].T)
        got["outimage"][s] = img[0].reshape(case.n_inframe, m).astype(np.float32)
        got["Tsum_stamp"][s], got["Tsum_inpix"][s], got["Neff"][s] = st[0], inpix[0].ravel(), neff.ravel()
    return got


def _emulate(case, data, defect=None):
    """The step in plain float64 numpy, with one of the index errors a kernel could make planted in it: last_row (a stamp with n % 16
    == 1 loses its last row), lost_flush (the first row group's sums of the first exposure run are dropped when the exposure changes),
    frame (frame f0 + f read as frame f), taper_twice (the second and later frame passes taper T again), column (output pixel m - 1
    taken from column m of Tt), neff_taper (Neff without its taper).  T itself is not returned: the sums must give the error away."""
    Tt, x, e = data
    batch, m, ne, nf = len(case.ns), case.m, case.n_expo, case.n_inframe
    got = dict(T=None, outimage=np.zeros((batch, nf, m), np.float32), Tsum_stamp=np.zeros((batch, ne)), Tsum_inpix=np.zeros((batch, m)),
               Neff=np.zeros((batch, m)))
    for s, ns in enumerate(case.ns):
        T = np.array(Tt[s, :ns, :m], np.float32, order="C")
        if defect == "column":
            T[:, m - 1] = Tt[s, :ns, m]
        orc.trapezoid(T.reshape(ns, case.n2f, case.n2f), case.fade)
        T2 = T.copy()
        orc.trapezoid(T2.reshape(ns, case.n2f, case.n2f), case.fade)
        es, keep = e[s, :ns], np.ones(ns, bool)
        if defect == "last_row" and ns % 16 == 1:
            keep[-1] = False
        if defect == "lost_flush" and ns > 0 and (es != es[0]).any():
            run = np.arange(ns) < np.argmax(es != es[0])
            keep &= ~(run & (np.arange(ns) % 4 == 0))
        T64 = T.astype(np.float64)
        v = np.stack([T64[keep & (es == q)].sum(axis=0) for q in range(ne)], axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            neff = 1.0 / np.square(v / np.abs(v).sum(axis=1)[:, None]).sum(axis=1)
        if defect != "neff_taper":
            orc.trapezoid(neff.reshape(case.n2f, case.n2f), case.fade)
        got["Tsum_inpix"][s], got["Tsum_stamp"][s], got["Neff"][s] = v.sum(axis=1), v.sum(axis=0) / case.n2**2, neff
        for f in range(nf):
            xf = x[s, f % 4 if defect == "frame" else f, :ns].astype(np.float64)
            Tf = (T2 if defect == "taper_twice" and f >= 4 else T).astype(np.float64)
            got["outimage"][s, f] = (xf[keep] @ Tf[keep]).astype(np.float32)
    return got


def test_reference_reproduces_the_recorded_coaddition(golden):
    """On the inputs of the golden stamp (the two target PSFs as a batch of two): the taper of T bit for bit; the sums within the
    tolerances tests/test_gpu_select.py holds the device to (the recorded ones are float32 segment sums, coadd.py:1329-1337)."""
    g = golden("coadd_stamp")
    nine, pivots = [], []
    bottom, top, left, right = (int(v) for v in g["sel_box"])
    for j, i in g["sel_order"]:
        nine.append((g[f"in{j}{i}_x"], g[f"in{j}{i}_y"], g[f"in{j}{i}_data"], g[f"in{j}{i}_cum"]))
        pivots.append(([left - 0.5, None, right + 0.5][i - 2 + 1], [bottom - 0.5, None, top + 0.5][j - 2 + 1]))
    _, _, indata, expo, cum = orc.process_input_stamps(nine, pivots, float(g["sel_rpix"]))
    assert np.array_equal(indata, g["sel_data"]) and np.array_equal(cum, g["sel_cumsum"])
    n2, fade, n_expo, n_inframe = (int(v) for v in g["co_pars"])
    n2f, n_out, N = n2 + 2 * fade, g["co_T_in"].shape[0], g["co_T_in"].shape[2]
    m, ldn, ldm = n2f * n2f, 256, 128
    Tt = np.zeros((n_out, ldn, ldm), np.float32)
    Tt[:, :N, :m] = g["co_T_in"].transpose(0, 2, 1)
    x = np.zeros((n_out, n_inframe, ldn), np.float32)
    x[:, :, :N] = indata
    e = np.zeros((n_out, ldn), np.int32)
    e[:, :N] = expo
    ref = ep.reference(Tt, x, e, [N] * n_out, n_expo, n2f, n2, fade)
    for o in range(n_out):
        assert np.array_equal(ref["T"][o].T, g["co_T_out"][o])
        img = g["co_outimage"][o].reshape(n_inframe, m)
        assert np.abs(ref["outimage"][o] - img).max() <= 1e-6 * np.abs(img).max()
        assert np.allclose(ref["Tsum_stamp"][o].astype(np.float64), g["co_Tsum_stamp"][o], rtol=1e-6, atol=0)
        assert np.allclose(ref["Tsum_inpix"][o].astype(np.float64), g["co_Tsum_inpix"][o].ravel(), rtol=0, atol=2e-7 * np.abs(g["co_Tsum_inpix"][o]).max())
        assert np.allclose(ref["Neff"][o].astype(np.float64), g["co_Neff"][o].ravel(), rtol=2e-6, atol=0)


@pytest.mark.parametrize("case", ep.CASES, ids=lambda c: c.name)
def test_numpy_in_float64_lies_within_the_bounds(case):
    """oracle.perform_coaddition in float64, and the plain float64 statement the planted defects are made from, for every stamp of
    every case; in the exact family the float64 sums ARE the long-double sums."""
    data = case.inputs()
    ref = case.reference(data)
    for got in (_oracle_f64(case, data), _emulate(case, data)):
        worst = ep.compare(got, ref, case)
        assert max(worst.values()) <= 1.0, (case.name, ep.fmt(worst))
        if case.exact:
            assert np.array_equal(got["Tsum_inpix"].astype(LD), ref["Tsum_inpix"])
            assert np.array_equal(got["outimage"], ref["outimage"].astype(np.float32))
            assert np.array_equal(got["Tsum_stamp"], (ref["v"].sum(axis=1).astype(np.float64)) / case.n2**2)  # exact sum, one division


def test_the_cap_on_the_inputs_holds():
    """S / sabs <= 4 at every pixel of every case outside the exact family -- the fused cases on the T numpy solves for them."""
    seen = 0
    for case in ep.CASES + ep.FUSED_CASES + [ep.REPAIR_CONTROL, ep.REPAIR_TWO_NODES]:
        if case.exact:
            continue
        if isinstance(case, ep.FusedCase):
            data = case.inputs()
            ref = ep.reference(case.host_T(data), data[3], data[4], case.ns, case.n_expo, case.n2f, case.n2, 0)
        else:
            ref = case.reference()
        for s, ns in enumerate(case.ns):
            if ns:
                assert (ref["sabs"][s] > 0).all() and float((ref["S"][s] / ref["sabs"][s]).max()) <= ep.CAP, (case.name, s)
                seen += 1
    assert seen > 50


def test_cases_are_what_they_claim():
    """The lane, frame and exposure edges are in the table; the special exposure patterns do what their names say."""
    c = BY_NAME
    assert {k.m for k in ep.CASES} >= {1, 4, 9, 64, 256, 289}
    assert {(k.n_expo, k.n_inframe) for k in ep.CASES} >= {(1, 1), (1, 4), (2, 5), (6, 2), (8, 8), (9, 3), (9, 9), (64, 1)}
    assert c["rows-ldn200"].ldn == max(c["rows-ldn200"].ns) == 200
    e = {p: ep.exposures(p, 33, 4) for p in ("runs", "missing", "alternate", "back", "single")}
    assert (np.diff(e["runs"]) >= 0).all() and set(e["runs"]) == {0, 1, 2, 3}
    assert set(e["missing"]) == {0, 1, 3}
    assert (np.diff(e["alternate"]) != 0).all() and all((np.diff(e["alternate"][r::4]) != 0).all() for r in range(4))
    cuts = np.flatnonzero(np.diff(e["back"]))
    assert e["back"][cuts[1] + 1] == e["back"][0] and e["back"][-1] == e["back"][cuts[0] + 1]
    ref = c["pattern-single"].reference()
    assert np.all(ref["Neff"] == 1)
    ref = c["pattern-zerocol"].reference()
    z = c["pattern-zerocol"].zero_col
    assert np.isnan(ref["Neff"][0, z]) and np.isnan(ref["Neff"][0]).sum() == 1
    assert ref["Tsum_inpix"][0, z] == 0 and np.all(ref["outimage"][0, :, z] == 0)
    ref = c["rows"].reference()
    assert np.isnan(ref["Neff"][0]).all() and not ref["outimage"][0].any() and not ref["Tsum_stamp"][0].any()  # n = 0
    for n2, fade in ep.FADES[:2]:
        assert n2 < 2 * fade


@pytest.mark.parametrize("defect,name", [("last_row", "rows"), ("lost_flush", "pattern-runs"), ("lost_flush", "fade-10-3-f1"), ("frame", "expo-2-5"),
                                         ("frame", "fade-8-1-f9"), ("taper_twice", "fade-10-3-f9"), ("taper_twice", "fade-1-1-f9"),
                                         ("column", "cols-3-e3"), ("column", "cols-17-e9"), ("neff_taper", "fade-8-1-f1"),
                                         ("neff_taper", "fade-2-3-f1")])
def test_comparator_rejects_planted_defects(defect, name):
    case = BY_NAME[name]
    Tt, x, e = case.inputs()
    if defect == "column":
        assert case.ldm > case.m
        Tt[:, :, case.m] = Tt[:, :, 0]  # (what a kernel reading one column too far would find there)
    ref = case.reference((Tt, x, e))
    assert max(ep.compare(_emulate(case, (Tt, x, e)), ref, case).values()) <= 1.0
    worst = ep.compare(_emulate(case, (Tt, x, e), defect), ref, case)
    assert max(worst.values()) > 1.0, (defect, name, ep.fmt(worst))
