"""The device WCS (seam 16) on the GPU: pyimcom_amd.wcs against the 40-digit fixture tests/golden/wcs.npz with the bound
|device - exact| <= 10 ref_err per case and quantity (ref_err: the float64 numpy restatement's own distance from the 40-digit value, capped in
tests/test_wcs_host.py), against the restatement where the check is an equality of masks and counts, and DestripeEngine.set_pair(wcs=).
astropy is not installed where this was written: the comparison with it is the last test and has not run."""

import json
import os

import numpy as np
import pytest

from tests import wcs_reference as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(ROOT, "tests", "golden", "wcs.npz"))
META = json.loads(str(G["meta"]))
CASES = {c["name"]: c for c in META["cases"]}
SIZES = (1, 63, 64, 65, 1027)
_CACHE = {}


def table_of(case):
    if not case["table"]:
        return None
    return (G["table_" + case["table"]], float(G["table_ends"][0]), float(G["table_ends"][1]))


def dev_wcs(name, nside=None):
    from pyimcom_amd import wcs as W

    key = (name, nside)
    if key not in _CACHE:
        c = CASES[name]
        n = nside or c["nside"]
        _CACHE[key] = W.DeviceWCS.from_header(c["header"], array_shape=(n, n), table=table_of(c), niter=c["niter"])
        assert np.array_equal(_CACHE[key].descriptor, G[name + "_desc"])
    return _CACHE[key]


def sizes_for(n):
    return [s for s in SIZES if s <= n] + [n]


def report(label, err, bound):
    print(f"{label}: largest error {np.max(err):.3e}, bound {bound:.3e}, ratio {np.max(err) / bound:.3f}")


@pytest.mark.parametrize("name", sorted(CASES))
def test_pix2world_and_world2pix_against_the_fixture(name):
    c, w = CASES[name], dev_wcs(name)
    pix, world, inv = G[name + "_pix"], G[name + "_world"], G[name + "_inv"]
    werr, ierr = 10 * G[name + "_world_err"], 10 * G[name + "_inv_err"]
    for n in sizes_for(len(pix)):
        got = w.all_pix2world(pix[:n], c["origin"])
        assert isinstance(got, np.ndarray) and got.shape == (n, 2) and got.dtype == np.float64
        assert np.all((got[:, 0] >= 0) & (got[:, 0] < 360))
        e0, e1 = R.ra_distance(got[:, 0], world[:n, 0]), np.abs(got[:, 1] - world[:n, 1])
        back = w.all_world2pix(world[:n], c["origin"])
        f0, f1 = np.abs(back[:, 0] - inv[:n, 0]), np.abs(back[:, 1] - inv[:n, 1])
        if n == len(pix):
            report(f"{name} ra", e0, werr[0]), report(f"{name} dec", e1, werr[1]), report(f"{name} x", f0, ierr[0]), report(f"{name} y", f1, ierr[1])
            trip = w.all_world2pix(got, c["origin"])
            print(f"{name}: round trip pix -> world -> pix {np.max(np.abs(trip - pix)):.3e} pixel (reported, not gated)")
        assert np.all(e0 <= werr[0]) and np.all(e1 <= werr[1]), (n, e0.max() / werr[0], e1.max() / werr[1])
        assert np.all(f0 <= ierr[0]) and np.all(f1 <= ierr[1]), (n, f0.max() / ierr[0], f1.max() / ierr[1])
    # the 3-argument forms give the same bits; a device tensor in gives a device tensor out
    import torch

    ra, dec = w.all_pix2world(pix[:65, 0].copy(), pix[:65, 1].copy(), c["origin"])
    full = w.all_pix2world(pix[:65], c["origin"])
    assert np.array_equal(ra, full[:, 0]) and np.array_equal(dec, full[:, 1])
    s = w.all_pix2world(float(pix[3, 0]), float(pix[3, 1]), c["origin"])
    assert s == (full[3, 0], full[3, 1])
    t = w.all_world2pix(torch.as_tensor(world[:65]).cuda(), c["origin"])
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), w.all_world2pix(world[:65], c["origin"]))
    t = w.all_world2pix(torch.as_tensor(world[:65]), c["origin"])  # a tensor in host memory: a tensor out, in host memory
    assert isinstance(t, torch.Tensor) and not t.is_cuda and np.array_equal(t.numpy(), w.all_world2pix(world[:65], c["origin"]))


@pytest.mark.parametrize("pair", [p["name"] for p in META["pairs"]])
def test_pix2pix_point_lists_against_the_fixture(pair):
    from pyimcom_amd import wcs as W

    p = [q for q in META["pairs"] if q["name"] == pair][0]
    a, b = dev_wcs(p["from"]), dev_wcs(p["to"])
    pix, xy, bound = G[p["from"] + "_pix"], G[pair + "_xy"], 10 * G[pair + "_err"]
    nside = CASES[p["to"]]["nside"]
    for n in sizes_for(len(pix)):
        x, y, m, counts = W._pix2pix(a, b, points=pix[:n], nside=nside, pad=2, origin=p["origin"])
        x, y, m = x.cpu().numpy(), y.cpu().numpy(), m.cpu().numpy()
        e0, e1 = np.abs(x - xy[:n, 0]), np.abs(y - xy[:n, 1])
        if n == len(pix):
            report(f"{pair} x", e0, bound[0]), report(f"{pair} y", e1, bound[1])
        assert np.all(e0 <= bound[0]) and np.all(e1 <= bound[1]), (n, e0.max() / bound[0], e1.max() / bound[1])
        assert np.array_equal(m.astype(bool), R.is_in_ref(x, y, nside, 2)) and counts == (int(np.count_nonzero(m)), 0)
        only = W._pix2pix(a, b, points=pix[:n], nside=nside, pad=2, origin=p["origin"], want="")
        assert only[:3] == (None, None, None) and only[3] == counts


def test_map_sca2sca_grids_masks_counts_and_casts():
    """nside = 250, pad = 3, subsamp 7 (37 x 37 points: a ragged last tile) against the fixture and as a subset of subsamp 1; the mask with ==
    from the device's own float64 positions; the float32 output; count-only; pad = 2 (254 x 254 points, no multiple of the 1024-point
    tile either) against the restatement."""
    from pyimcom_amd import wcs as W

    g = META["grid"]
    a, b = dev_wcs(g["target"]), dev_wcs(g["ref"])
    nside, pad = CASES[g["target"]]["nside"], g["pad"]
    x7, y7, m7 = W.map_sca2sca(a, b, pad=pad, subsamp=g["subsamp"])
    assert x7.shape == y7.shape == m7.shape == (37, 37) and x7.dtype == np.float64 and m7.dtype == bool
    bound = 10 * G["grid_err"]
    e0, e1 = np.abs(x7.ravel() - G["grid_xy"][:, 0]), np.abs(y7.ravel() - G["grid_xy"][:, 1])
    report("grid x", e0, bound[0]), report("grid y", e1, bound[1])
    assert np.all(e0 <= bound[0]) and np.all(e1 <= bound[1])
    x1, y1, m1 = W.map_sca2sca(a, b, pad=pad, subsamp=1)
    assert x1.shape == (nside + 2 * pad,) * 2
    k = g["subsamp"] // 2
    assert np.array_equal(x1[k::7, k::7], x7) and np.array_equal(y1[k::7, k::7], y7) and np.array_equal(m1[k::7, k::7], m7)  # the same bits in any chunking
    xr, yr, mr = R.np_map_sca2sca(a.descriptor, None, b.descriptor, None, nside, pad, 1)
    assert np.max(np.abs(x1 - xr)) <= 11 * G["grid_err"][0] and np.max(np.abs(y1 - yr)) <= 11 * G["grid_err"][1]
    for x, y, m, sub in ((x1, y1, m1, 1), (x7, y7, m7, 7)):
        assert np.array_equal(m, R.is_in_ref(x, y, nside, pad)) and 0 < np.count_nonzero(m) < m.size
        inside, size = W.overlap_count(a, b, pad=pad, subsamp=sub)
        assert (inside, size) == (int(np.count_nonzero(m)), m.size)
        xs, ys, ms = W.map_sca2sca(a, b, pad=pad, subsamp=sub, dtype=np.float32)
        assert xs.dtype == np.float32 and np.array_equal(xs, x.astype(np.float32)) and np.array_equal(ys, y.astype(np.float32)) and np.array_equal(ms, m)
    x2, y2, m2 = W.map_sca2sca(a, b, pad=2, subsamp=1)
    xr, yr, mr = R.np_map_sca2sca(a.descriptor, None, b.descriptor, None, nside, 2, 1)
    assert x2.shape == (254, 254) and np.max(np.abs(x2 - xr)) <= 11 * G["grid_err"][0] and np.max(np.abs(y2 - yr)) <= 11 * G["grid_err"][1]
    assert np.array_equal(m2, R.is_in_ref(x2, y2, nside, 2)) and W.overlap_count(a, b, pad=2) == (int(np.count_nonzero(m2)), m2.size)
    xd, yd, md = W.map_sca2sca(a, b, pad=pad, subsamp=1, device_out=True)
    assert xd.is_cuda and np.array_equal(xd.cpu().numpy(), x1) and md.dtype.is_floating_point is False and np.array_equal(md.cpu().numpy(), m1)


def test_mask_at_points_within_an_ulp_of_the_edges():
    """Two plain TAN chips with one CRVAL = (0, 0), for which the rotation between them is the identity exactly: the target's pixel (0, 0) and
    the reference's pixel (-0.5 - pad, -0.5 - pad) both sit on CRVAL, so a target pixel d maps to the edge + d with d resolved far below an
    ulp of the edge.  The mask is the reference's expression, evaluated by numpy on the device's float64 outputs, with ==: strict in x, not
    strict in y."""
    from pyimcom_amd import wcs as W

    nside, pad = 250, 3
    edge = -0.5 - pad
    s = 0.11 / 3600.0
    base = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CRVAL1": 0.0, "CRVAL2": 0.0, "CD1_1": s, "CD1_2": 0.0, "CD2_1": 0.0, "CD2_2": s}
    tgt = W.DeviceWCS.from_header({**base, "CRPIX1": 1.0, "CRPIX2": 1.0}, array_shape=(nside, nside))
    ref = W.DeviceWCS.from_header({**base, "CRPIX1": edge + 1.0, "CRPIX2": edge + 1.0}, array_shape=(nside, nside))
    Rm = tgt.descriptor[R.D_ROT:R.D_ROT + 9].reshape(3, 3)
    assert np.array_equal(Rm @ Rm.T, np.eye(3))
    d = np.arange(-8, 9) * 2.0 ** -53  # a quarter of an ulp of 3.5 apart
    pts = np.concatenate((np.stack((d, np.full_like(d, 50.0)), 1), np.stack((np.full_like(d, 50.0), d), 1)))
    x, y, m, counts = W._pix2pix(tgt, ref, points=pts, nside=nside, pad=pad)
    x, y, m = x.cpu().numpy(), y.cpu().numpy(), m.cpu().numpy().astype(bool)
    half = len(d)
    ulp = np.spacing(abs(edge))
    print(f"distances from the x edge in ulps: {np.unique((x[:half] - edge) / ulp)}, from the y edge: {np.unique((y[half:] - edge) / ulp)}")
    assert np.max(np.abs(x[:half] - edge)) <= 2 * ulp and np.max(np.abs(y[half:] - edge)) <= 2 * ulp
    for v in (x[:half], y[half:]):
        assert (v == edge).any() and (v == edge - ulp).any() and (v == edge + ulp).any()  # on it, one ulp outside, one ulp inside
    assert np.array_equal(m, R.is_in_ref(x, y, nside, pad)) and counts == (int(np.count_nonzero(m)), 0)
    assert not m[:half][x[:half] <= edge].any() and m[:half][x[:half] > edge].all()  # strict in x
    assert not m[half:][y[half:] < edge].any() and m[half:][y[half:] >= edge].all()  # not strict in y
    # and on a whole grid: the reference chip shifted by half a pixel plus the pad, whose first column and row straddle the edges
    ref2 = W.DeviceWCS.from_header({**base, "CRPIX1": 1.0 - (0.5 + pad) + pad, "CRPIX2": 1.0 - (0.5 + pad) + pad}, array_shape=(nside, nside))
    xf, yf, mm = W.map_sca2sca(tgt, ref2, pad=pad)
    assert np.array_equal(mm, R.is_in_ref(xf, yf, nside, pad)) and np.abs(xf[:, 0] - edge).max() < 1e-9 and 0 < np.count_nonzero(mm) < mm.size


def test_far_hemisphere_antipode_and_nan_are_written_nan_and_counted():
    from pyimcom_amd import wcs as W

    tan, stg = dev_wcs("sip2_m40"), dev_wcs("stg_m40")
    h = CASES["sip2_m40"]["header"]
    world = np.array([[h["CRVAL1"] + 180.0, -h["CRVAL2"]], [h["CRVAL1"], h["CRVAL2"] + 90.0], [h["CRVAL1"] + 100.0, 30.0], [np.nan, 0.0], [10.0, np.inf],
                      [h["CRVAL1"], h["CRVAL2"]]])
    pix, nbad = tan._list(1, world, 0, count_bad=True)
    assert np.isnan(pix[:5]).all() and np.isfinite(pix[5]).all() and nbad == 5
    hs = CASES["stg_m40"]["header"]
    ws = np.array([[hs["CRVAL1"] + 180.0, -hs["CRVAL2"]], [hs["CRVAL1"] + 100.0, 30.0], [np.nan, np.nan]])
    pix, nbad = stg._list(1, ws, 1, count_bad=True)
    assert np.isnan(pix[0]).all() and np.isfinite(pix[1]).all() and np.isnan(pix[2]).all() and nbad == 2  # STG serves the far hemisphere, not the antipode
    out, nbad = tan._list(0, np.array([[np.nan, 1.0], [1.0, 2.0], [np.inf, 5.0]]), 0, count_bad=True)
    assert np.isnan(out[0]).all() and np.isfinite(out[1]).all() and np.isnan(out[2]).all() and nbad == 2
    # a chip on the other side of the sky: every point NaN, none inside, all counted
    far = W.DeviceWCS.from_header({**h, "CRVAL1": h["CRVAL1"] + 180.0, "CRVAL2": -h["CRVAL2"]}, array_shape=(250, 250))
    near = W.DeviceWCS.from_header(h, array_shape=(250, 250))
    x, y, m = W.map_sca2sca(near, far, pad=0, subsamp=7)
    assert np.isnan(x).all() and np.isnan(y).all() and not m.any()
    g = [3.0, 7.0, 36, 3.0, 7.0, 36]
    assert W._pix2pix(near, far, grid=g, nside=250, want="")[3] == (0, 36 * 36)
    tab = dev_wcs("tab32_n3")
    x, y, m, counts = W._pix2pix(tab, tab, points=np.array([[np.nan, 3.0], [4.0, 5.0]]), nside=48)
    assert np.isnan(x[0].item()) and np.isfinite(x[1].item()) and counts == (1, 1)


def test_overlap_matrix_of_five_small_chips():
    from pyimcom_amd import wcs as W

    names = ["small_a", "small_b", "small_c", "small_d", "small_e"]
    ws = [dev_wcs(n) for n in names]
    want = R.np_overlap_matrix([G[n + "_desc"] for n in names], 250, pad=2, subsamp=3)
    got = W.get_overlap_matrix(ws, pad=2, subsamp=3)
    assert got.dtype == np.float32 and got.shape == (5, 5) and np.array_equal(got, want), (got, want)
    assert np.all(got[3, :3] == 0) and np.all(got[4, :4] == 0) and np.all(np.diag(got) == 1) and 0 < got[1, 0] < 1 and np.array_equal(got, got.T)
    caps = [W.footprint_cap(w, 2.0) for w in ws]
    touch = W.caps_can_touch(np.array([c[0] for c in caps]), [c[1] for c in caps])
    assert np.array_equal(touch, want > 0)  # the disjoint chips never reach a launch


@pytest.mark.parametrize("area", [a["name"] for a in META["areas"]])
def test_pix_area_against_the_fixture(area):
    from pyimcom_amd import wcs as W

    a = [q for q in META["areas"] if q["name"] == area][0]
    info = {}
    got = W.pix_area(dev_wcs(a["case"]), a["region"], pad=a["pad"], ovsamp=a["ovsamp"], info=info)
    ex, bound = G[area + "_area"], 10 * G[area + "_err"][0]
    assert got.shape == ex.shape and got.dtype == np.float64 and info["rotated"] == a["turned"]
    report(area, np.abs(got - ex), bound)
    assert np.all(np.abs(got - ex) <= bound)


def test_destripe_pair_from_two_wcs_equals_the_uploaded_arrays():
    import torch

    from pyimcom_amd import wcs as W
    from pyimcom_amd.destripe import DestripeEngine

    nside = 64
    h0, h1 = dict(CASES["small_a"]["header"]), dict(CASES["small_b"]["header"])
    for h in (h0, h1):
        h["CRPIX1"] = h["CRPIX2"] = 32.5
    h1["CRVAL1"], h1["CRVAL2"] = h0["CRVAL1"] + 0.0006, h0["CRVAL2"] + 0.0004  # about 20 pixels apart
    w = [W.DeviceWCS.from_header(h, array_shape=(nside, nside)) for h in (h0, h1)]
    rng = np.random.default_rng(16)
    scas = [(rng.normal(100.0, 5.0, (nside, nside)).astype(np.float32), rng.random((nside, nside)) > 0.1, rng.uniform(0.9, 1.1, (nside, nside)).astype(np.float32))
            for _ in range(2)]

    def engine(how):
        eng = DestripeEngine(nside, nside)
        for s in scas:
            eng.add_sca(*s)
        for a, b in ((0, 1), (1, 0)):
            if how == "wcs":
                eng.set_pair(a, b, wcs=(w[a], w[b]))
            else:
                x, y, _ = W.map_sca2sca(w[a], w[b], pad=0)
                assert x.shape == (nside, nside)
                eng.set_pair(a, b, x=x, y=y)
        return eng

    e1, e2 = engine("wcs"), engine("arrays")
    assert e1.plan() == e2.plan() and e1.plan()["pairs_full"] > 0
    n1, n2 = e1.N_eff.cpu().numpy(), e2.N_eff.cpu().numpy()
    assert np.array_equal(n1, n2) and n1.max() > 0
    params = rng.normal(0.0, 1.0, (2, e1.nbins))
    c1, psi1 = e1.cost(params)
    c2, psi2 = e2.cost(params)
    assert c1 == c2 and torch.equal(psi1, psi2)
    assert np.array_equal(e1.residual(psi1), e2.residual(psi2))
    with pytest.raises(ValueError):
        e1.set_pair(0, 1, x=np.zeros((nside, nside)), y=np.zeros((nside, nside)), wcs=(w[0], w[1]))
    with pytest.raises(ValueError):
        e1.set_pair(0, 1, lattice=np.zeros((2, 5, 5)), wcs=(w[0], w[1]))


def test_c_abi_refusals():
    import ctypes as C

    from pyimcom_amd import _lib
    from pyimcom_amd import wcs as W

    import torch

    ctx = _lib.default_context(0)
    d = dev_wcs("tan_m40").descriptor.copy()
    pts = torch.zeros((4, 2), dtype=torch.float64, device="cuda")
    out = torch.empty_like(pts)

    def call(desc, n=4, origin=0):
        return _lib.lib.imcom_wcs_pix2world(ctx.handle, _lib.ptr(desc), None, 0, 0, 0.0, 0.0, _lib.ptr(pts), n, origin, _lib.ptr(out), None, _lib.MEM_DEVICE)

    assert call(d) == 0
    for k, v, status in ((W.D_PROJ, 2.0, -4), (W.D_AORDER, 10.0, -4), (W.D_BORDER, 1.5, -1), (W.D_NITER, 99.0, -1), (W.D_CD, np.nan, -1)):
        bad = d.copy()
        bad[k] = v
        assert call(bad) == status, (k, v)
    sing = d.copy()
    sing[W.D_CD:W.D_CD + 4] = [1e-5, 2e-5, 2e-5, 4e-5]
    assert call(sing) == -1 and call(d, origin=2) == -1 and call(d, n=-1) == -1 and call(d, n=0) == 0
    for kw in (dict(nside=float("nan")), dict(pad=float("inf"))):
        with pytest.raises(_lib.ImcomError) as e:
            W._pix2pix(dev_wcs("small_a"), dev_wcs("small_b"), grid=[0.0, 1.0, 8, 0.0, 1.0, 8], **{"nside": 250, **kw})
        assert e.value.status == -1
    sz = (C.c_long * 4)()
    assert _lib.lib.imcom_wcs_sizes(10, 8, 8, sz) == 0 and sz[2] == W.DESC_LEN and sz[3] == W.MAX_ORDER
    # host arrays go through the workspace and give the same bits
    c = CASES["tab64_n1"]
    w = dev_wcs("tab64_n1")
    pix = np.ascontiguousarray(G["tab64_n1_pix"][:65])
    host = np.empty_like(pix)
    tab = np.ascontiguousarray(w.table[0])
    nbad = C.c_long(-1)
    _lib.check(_lib.lib.imcom_wcs_pix2world(ctx.handle, _lib.ptr(w.descriptor), _lib.ptr(tab), 1, tab.shape[1], w.table[1], w.table[2], _lib.ptr(pix), 65, c["origin"],
                                            _lib.ptr(host), C.byref(nbad), _lib.MEM_HOST))
    assert nbad.value == 0 and np.array_equal(host, w.all_pix2world(pix, c["origin"]))


def test_against_astropy_when_it_is_installed():
    """Has not run where this was written (astropy is not installed there).  all_pix2world at 1e-9 degree; all_world2pix at 2e-4 pixel, astropy's
    own tolerance being 1e-4."""
    pytest.importorskip("astropy")
    from astropy.io import fits
    from astropy.wcs import WCS

    from pyimcom_amd import wcs as W

    c = CASES["sip2_m40"]
    hdr = fits.Header()
    for k, v in c["header"].items():
        hdr[k] = v
    aw = WCS(hdr)
    pix = G["sip2_m40_pix"][:300]
    for w in (W.DeviceWCS.from_header(hdr), W.DeviceWCS.from_astropy(aw)):
        assert np.array_equal(w.descriptor, G["sip2_m40_desc"])
        world = w.all_pix2world(pix, 0)
        want = aw.all_pix2world(pix, 0)
        assert np.max(R.ra_distance(world[:, 0], want[:, 0])) < 1e-9 and np.max(np.abs(world[:, 1] - want[:, 1])) < 1e-9
        assert np.max(np.abs(w.all_world2pix(want, 0) - aw.all_world2pix(want, 0))) < 2e-4
