"""CPU-side checks of the device WCS (seam 16): the float64 numpy restatement that the device tests lean on (tests/wcs_reference.py) against
the 40-digit fixture, with the caps that keep a loose ``ref_err`` from hiding a failure; the error map against scipy's
``RegularGridInterpolator`` built exactly as ``LocWCS.err_interp`` builds it; the three constructors of ``DeviceWCS``; the argument forms of
its two methods; and csrc/wcs_core.h as a host program under the sanitizers.  astropy is not installed here: nothing in this file compares
with astropy."""

import json
import os
import subprocess

import numpy as np
import pytest

from tests import wcs_reference as R
from tests.conftest import ROOT

G = np.load(os.path.join(ROOT, "tests", "golden", "wcs.npz"))
META = json.loads(str(G["meta"]))
CASES = {c["name"]: c for c in META["cases"]}
EPS = np.finfo(np.float64).eps
WORLD_CAP = 64 * EPS * 360.0  # degrees


def table_of(case):
    if not case["table"]:
        return None
    return (G["table_" + case["table"]], float(G["table_ends"][0]), float(G["table_ends"][1]))


def pixel_cap(desc):
    return 64 * EPS / R.pixel_scale_rad(desc)


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_against_the_fixture_and_the_caps(name):
    c, d, tab = CASES[name], G[name + "_desc"], table_of(CASES[name])
    pix, world, inv = G[name + "_pix"], G[name + "_world"], G[name + "_inv"]
    ra, dec = R.np_pix2world(d, tab, pix[:, 0], pix[:, 1], c["origin"])
    assert np.all((ra >= 0) & (ra < 360))
    # the stored ref_err is the restatement's distance from the 40-digit value; from the rounded value it is at most half an ulp further
    assert np.max(R.ra_distance(ra, world[:, 0])) <= G[name + "_world_err"][0] + 360 * EPS
    assert np.max(np.abs(dec - world[:, 1])) <= G[name + "_world_err"][1] + 90 * EPS
    x, y, ok = R.np_world2pix(d, tab, world[:, 0], world[:, 1], c["origin"])
    assert ok.all()
    assert np.max(np.abs(x - inv[:, 0])) <= G[name + "_inv_err"][0] + 8192 * EPS and np.max(np.abs(y - inv[:, 1])) <= G[name + "_inv_err"][1] + 8192 * EPS
    assert np.all(G[name + "_world_err"] < WORLD_CAP), G[name + "_world_err"]
    assert np.all(G[name + "_inv_err"] < pixel_cap(d)), (G[name + "_inv_err"], pixel_cap(d))
    assert pix[0, 0] == c["header"]["CRPIX1"] - 1 + c["origin"]  # r = 0 is among the points
    assert np.max(np.abs(world[0] - [c["header"]["CRVAL1"], c["header"]["CRVAL2"]])) < 1e-12 or tab is not None


@pytest.mark.parametrize("pair", [p["name"] for p in META["pairs"]] + ["grid"])
def test_pixel_chains_against_the_fixture_and_the_caps(pair):
    if pair == "grid":
        g = META["grid"]
        a, b, origin = g["target"], g["ref"], 0
        s = R.grid_axis(CASES[a]["nside"], g["pad"], g["subsamp"])
        gx, gy = np.meshgrid(s, s)
        pix = np.stack((gx.ravel(), gy.ravel()), 1)
    else:
        p = [q for q in META["pairs"] if q["name"] == pair][0]
        a, b, origin = p["from"], p["to"], p["origin"]
        pix = G[a + "_pix"]
    x, y, ok = R.np_pix2pix(G[a + "_desc"], table_of(CASES[a]), G[b + "_desc"], table_of(CASES[b]), pix[:, 0], pix[:, 1], origin)
    assert ok.all()
    err = G[pair + "_err"]
    assert np.max(np.abs(x - G[pair + "_xy"][:, 0])) <= err[0] + 16384 * EPS and np.max(np.abs(y - G[pair + "_xy"][:, 1])) <= err[1] + 16384 * EPS
    assert np.all(err < pixel_cap(G[b + "_desc"])), (err, pixel_cap(G[b + "_desc"]))


def test_roman_scale_chains_stay_inside_the_bound_of_the_issue():
    """dec -40, dec 89.9 and ra 359.99: the restatement's distance from the 40-digit chain is below 64 eps / (0.11 arcsec) = 2.6e-8 pixel."""
    for pair in ("chain_m40", "chain_pole", "chain_wrap"):
        assert np.all(G[pair + "_err"] < 2.7e-8) and np.all(G[pair + "_err"] > 0)


def test_fixture_regenerates_where_mpmath_is_installed():
    pytest.importorskip("mpmath")
    for name in ("sip2_m40", "stg_pole", "sip4_wrap", "tab32_n3"):
        c, tab = CASES[name], table_of(CASES[name])
        P = R.header_params(c["header"])
        for k in (0, 1, 5, 40):
            x, y = G[name + "_pix"][k]
            ra, dec = R.mp_pix2world(P, tab, x, y, c["origin"])
            assert [float(ra), float(dec)] == list(G[name + "_world"][k])
            xi, yi = R.mp_world2pix(P, tab, c["niter"], *G[name + "_world"][k], c["origin"])
            assert [float(xi), float(yi)] == list(G[name + "_inv"][k])
    p = META["pairs"][0]
    a, b = CASES[p["from"]], CASES[p["to"]]
    for k in (0, 3, 77):
        x, y = G[a["name"] + "_pix"][k]
        xo, yo = R.mp_pix2pix(R.header_params(a["header"]), None, R.header_params(b["header"]), None, 0, x, y, p["origin"])
        assert [float(xo), float(yo)] == list(G[p["name"] + "_xy"][k])


def test_area_fixture_and_its_cap():
    """get_pix_area differences ra in degrees: its noise is about ulp(ra) / (ra step); the cap on the restatement's relative ref_err is the
    world cap over the pixel scale, 64 eps 360 / (0.11 arcsec in degrees) = 1.7e-7."""
    turned = []
    for a in META["areas"]:
        c = CASES[a["case"]]
        got, t = R.np_pix_area(G[c["name"] + "_desc"], None, a["region"], a["pad"], a["ovsamp"])
        turned.append(t)
        ex = G[a["name"] + "_area"]
        assert got.shape == ex.shape == (a["ovsamp"] * (a["region"][3] - a["region"][2]), a["ovsamp"] * (a["region"][1] - a["region"][0]))
        assert np.max(np.abs(got - ex)) <= G[a["name"] + "_err"][0] * (1 + 1e-9)
        assert G[a["name"] + "_err"][0] / ex.mean() < WORLD_CAP / (0.11 / 3600)
        assert abs(ex.mean() / (0.11 / 3600) ** 2 - 1) < 0.05
    assert turned == [False, True]  # the second footprint straddles ra = 0


# ---- the error map against scipy ----------------------------------------------------------------------------------------------------------

def _scipy_interpolators(table, lo, hi):
    """scipy's interpolators on the padded grid, with the arguments LocWCS.err_interp gives them (wcsutil.py:406-412): linear, no bounds error,
    extrapolating."""
    from scipy.interpolate import RegularGridInterpolator

    nodes = np.concatenate(([lo], np.arange(table.shape[1] - 2, dtype=np.float64), [hi]))
    return [RegularGridInterpolator((nodes, nodes), plane, method="linear", bounds_error=False, fill_value=None) for plane in table]


def _table_probes(N, n_pad):
    rng = np.random.default_rng(5)
    nodes = np.concatenate(([-n_pad], np.arange(N), [N + n_pad - 1])).astype(np.float64)
    on = np.stack(np.meshgrid(nodes, nodes), -1).reshape(-1, 2)
    wide = np.concatenate((rng.uniform(-n_pad, 0, (200, 2)), rng.uniform(N - 1, N + n_pad - 1, (200, 2)),
                           np.stack((rng.uniform(-n_pad, 0, 200), rng.uniform(0, N - 1, 200)), 1)))
    beyond = np.concatenate((rng.uniform(-3 * n_pad, -n_pad, (200, 2)), rng.uniform(N + n_pad - 1, N + 3 * n_pad, (200, 2)),
                             np.stack((rng.uniform(N + n_pad, N + 2 * n_pad, 100), rng.uniform(-2 * n_pad, -n_pad, 100)), 1)))
    inside = rng.uniform(0, N - 1, (500, 2))
    return np.concatenate((on, wide, beyond, inside))  # columns (x, y)


@pytest.mark.parametrize("use_float32", [True, False])
def test_error_map_against_scipy(use_float32):
    from pyimcom_amd import wcs as W

    table, lo, hi = W.error_table(G["errmap"], a=META["tab_a"], n_pad=META["tab_npad"], use_float32=use_float32)
    assert table.dtype == (np.float32 if use_float32 else np.float64) and table.shape == (2, 50, 50) and (lo, hi) == (-24.0, 71.0)
    assert np.array_equal(table, G["table_f32" if use_float32 else "table_f64"]) and [lo, hi] == list(G["table_ends"])
    # the padding is a straight line through the edge pixel and the pixel `a` further in, continued n_pad pixels out; corners from the padded columns
    e, (a_, n_pad) = G["errmap"].astype(table.dtype), (META["tab_a"], META["tab_npad"])
    assert np.array_equal(table[:, 1:-1, 1:-1], e)
    assert np.allclose(table[:, 1:-1, 0], e[:, :, 0] + (e[:, :, 0] - e[:, :, a_]) * n_pad / a_, rtol=1e-6, atol=1e-9)
    assert np.allclose(table[:, -1, 1:-1], e[:, -1, :] + (e[:, -1, :] - e[:, -1 - a_, :]) * n_pad / a_, rtol=1e-6, atol=1e-9)
    assert np.allclose(table[:, 0, 0], table[:, 1, 0] + (table[:, 1, 0] - table[:, 1 + a_, 0]) * n_pad / a_, rtol=1e-6, atol=1e-9)
    interps = _scipy_interpolators(table, lo, hi)
    xy = _table_probes(G["errmap"].shape[1], META["tab_npad"])
    dx, dy = R.np_table((table, lo, hi), xy[:, 0], xy[:, 1])
    yx = xy[:, ::-1]  # the interpolators take (y, x) columns
    # the bound: 8 eps sum |w_k| |v_k| over the four taps
    n2 = table.shape[1]
    ix, fx = R.np_cell(xy[:, 0], n2, lo, hi)
    iy, fy = R.np_cell(xy[:, 1], n2, lo, hi)
    for k, got in ((0, dx), (1, dy)):
        v = np.abs(table[k].astype(np.float64))
        bound = 8 * EPS * (v[iy, ix] * np.abs((1 - fy) * (1 - fx)) + v[iy, ix + 1] * np.abs((1 - fy) * fx) + v[iy + 1, ix] * np.abs(fy * (1 - fx))
                           + v[iy + 1, ix + 1] * np.abs(fy * fx))
        want = interps[k](yx)
        assert np.all(np.abs(got - want) <= bound), np.max(np.abs(got - want) / bound)
    assert np.isnan(R.np_table((table, lo, hi), np.array([np.nan, 1.0]), np.array([1.0, np.inf]))[0]).all()


# ---- packing ------------------------------------------------------------------------------------------------------------------------------

class _Obj:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _astropy_like(header, with_cd=True):
    """What from_astropy reads, hand-made from a header."""
    P = R.header_params(header)
    ww = _Obj(naxis=2, crpix=np.array(P["crpix"]), crval=np.array(P["crval"]), ctype=[header["CTYPE1"], header["CTYPE2"]],
              lonpole=header.get("LONPOLE", float("nan")))
    if with_cd:
        ww.cd = np.array(P["cd"]).reshape(2, 2)
    else:
        cdelt = np.array([0.5, 0.25])
        ww.cdelt = cdelt
        ww.pc = np.array(P["cd"]).reshape(2, 2) / cdelt[:, None]
    sip = None
    if P["a_order"] or P["b_order"]:
        a, b = np.zeros((P["a_order"] + 1,) * 2), np.zeros((P["b_order"] + 1,) * 2)
        for (p, q), v in P["a"].items():
            a[p, q] = v
        for (p, q), v in P["b"].items():
            b[p, q] = v
        sip = _Obj(a=a, b=b, a_order=P["a_order"], b_order=P["b_order"])
    return _Obj(wcs=ww, sip=sip, array_shape=None)


@pytest.mark.parametrize("name", ["tan_m40", "sip4_wrap", "sip4_wrap_b", "stg_m40", "tab32_n3"])
def test_the_three_constructors_give_one_descriptor(name):
    from pyimcom_amd import wcs as W

    c = CASES[name]
    shape = (c["nside"], c["nside"])
    tab = table_of(c)
    w1 = W.DeviceWCS.from_header(c["header"], array_shape=shape, table=tab, niter=c["niter"])
    assert np.array_equal(w1.descriptor, G[name + "_desc"]) and w1.descriptor.shape == (W.DESC_LEN,) == (R.DESC_LEN,)
    w2 = W.DeviceWCS.from_astropy(_astropy_like(c["header"]), array_shape=shape, table=tab, niter=c["niter"])
    assert np.array_equal(w2.descriptor, w1.descriptor)
    if tab is None:
        py = _Obj(type="ASTROPY", constructortype="FITSHEADER", obj=_astropy_like(c["header"]), array_shape=shape)
    else:
        ends = np.concatenate(([tab[1]], np.arange(tab[0].shape[1] - 2), [tab[2]]))
        py = _Obj(type="ASTROPY+", constructortype="GWCS", obj=_astropy_like(c["header"]), array_shape=shape, niter=c["niter"],
                  err=tuple(_Obj(grid=(ends, ends), values=tab[0][k]) for k in (0, 1)))
    w3 = W.DeviceWCS.from_pyimcom(py)
    assert np.array_equal(w3.descriptor, w1.descriptor) and w3.array_shape == shape and w3.constructortype == py.constructortype
    assert W.as_device_wcs(py).descriptor.tobytes() == w1.descriptor.tobytes() and W.as_device_wcs(w1) is w1
    if tab is not None:
        assert w3.type == "ASTROPY+" and np.array_equal(w3.table[0], tab[0]) and w3.table[0].dtype == tab[0].dtype and w3.table[1:] == tab[1:] and w3.niter == c["niter"]
    # the rotation is Paper II eq. (2): orthonormal, its third row the direction of CRVAL
    Rm = w1.descriptor[R.D_ROT:R.D_ROT + 9].reshape(3, 3)
    assert np.max(np.abs(Rm @ Rm.T - np.eye(3))) < 4 * EPS
    a, d = np.deg2rad(c["header"]["CRVAL1"]), np.deg2rad(c["header"]["CRVAL2"])
    assert np.max(np.abs(Rm[2] - [np.cos(d) * np.cos(a), np.cos(d) * np.sin(a), np.sin(d)])) < 4 * EPS


def test_packing_defaults_and_refusals():
    from pyimcom_amd import wcs as W
    from pyimcom_amd._lib import ImcomError

    h = dict(CASES["sip2_m40"]["header"])
    assert "LONPOLE" not in h
    assert np.array_equal(W.DeviceWCS.from_header(h).descriptor, W.DeviceWCS.from_header({**h, "LONPOLE": 180.0}).descriptor)
    assert W.DeviceWCS.from_header(h).lonpole == 180.0 and W.DeviceWCS.from_header({**h, "CRVAL2": 90.0}).lonpole == 0.0
    assert not np.array_equal(W.DeviceWCS.from_header(h).descriptor, W.DeviceWCS.from_header({**h, "LONPOLE": 137.0}).descriptor)
    assert W.DeviceWCS.from_header(h).array_shape == (4088, 4088)
    # NAXIS counts the data's axes: a cube with a two-axis celestial WCS is served; WCSAXES = 3 or a third axis' keys are not
    assert np.array_equal(W.DeviceWCS.from_header({**h, "NAXIS": 3, "NAXIS3": 5}).descriptor, W.DeviceWCS.from_header(h).descriptor)
    with pytest.raises(ImcomError):
        W.DeviceWCS.from_header({**h, "WCSAXES": 3})
    # PC + CDELT equals CD (powers of two: the products are exact), and CDELT alone is the diagonal
    cd = {"CD1_1": -2.0 ** -15, "CD1_2": 2.0 ** -17, "CD2_1": 2.0 ** -18, "CD2_2": 2.0 ** -15}
    base = {k: v for k, v in h.items() if not k.startswith("CD")}
    pc = {"CDELT1": 2.0 ** -15, "CDELT2": 2.0 ** -16, "PC1_1": -1.0, "PC1_2": 0.25, "PC2_1": 0.25, "PC2_2": 2.0}
    assert np.array_equal(W.DeviceWCS.from_header({**base, **cd}).descriptor, W.DeviceWCS.from_header({**base, **pc}).descriptor)
    assert np.array_equal(W.DeviceWCS.from_astropy(_astropy_like(h, with_cd=False)).descriptor, W.DeviceWCS.from_header(h).descriptor)
    only = W.DeviceWCS.from_header({**base, "CDELT1": -3e-5, "CDELT2": 3e-5}).descriptor
    assert list(only[R.D_CD:R.D_CD + 4]) == [-3e-5, 0.0, 0.0, 3e-5]
    # A_ORDER != B_ORDER, and where a coefficient goes
    d = G["sip4_wrap_desc"]
    assert (d[R.D_AORDER], d[R.D_BORDER]) == (4, 3) and d[R.D_A + R.sip_index(1, 3)] == CASES["sip4_wrap"]["header"]["A_1_3"]
    assert d[R.D_B + R.sip_index(2, 1)] == CASES["sip4_wrap"]["header"]["B_2_1"] and W.sip_index(9, 0) == R.sip_index(9, 0) == 54
    for bad in ({"CTYPE1": "RA---SIN", "CTYPE2": "DEC--SIN"}, {"PV2_1": 0.1}, {"CTYPE3": "WAVE"}, {"A_ORDER": 10}, {"CPDIS1": "LOOKUP"}, {"CROTA2": 3.0},
                {"CTYPE1": "GLON-TAN", "CTYPE2": "GLAT-TAN"}):
        with pytest.raises(ImcomError) as e:
            W.DeviceWCS.from_header({**h, **bad})
        assert e.value.status == -4, bad
    with pytest.raises(TypeError):
        W.DeviceWCS.from_pyimcom(_Obj(type="GWCS", constructortype="GWCS", obj=object()))


def test_argument_forms_of_the_two_methods(monkeypatch):
    """wcsutil.py:524-560 / 598-634: (pos, origin) and (pos, pos2, origin), scalars included -- shapes and types only, no device call."""
    from pyimcom_amd import wcs as W

    seen = []

    def fake(self, inverse, pos, origin, ctx=None, count_bad=False):
        assert isinstance(pos, np.ndarray) and pos.dtype == np.float64 and pos.ndim == 2 and pos.shape[1] == 2
        seen.append((inverse, pos.shape[0], origin))
        return pos + 1.0

    monkeypatch.setattr(W.DeviceWCS, "_list", fake)
    w = W.DeviceWCS.from_header(CASES["tan_m40"]["header"])
    for method, inverse in ((w.all_pix2world, 0), (w.all_world2pix, 1)):
        o = method(np.zeros((7, 2)), 0)
        assert o.shape == (7, 2) and o.dtype == np.float64
        o = method([[1, 2], [3, 4]], 1)
        assert o.shape == (2, 2) and seen[-1] == (inverse, 2, 1)
        a, b = method(np.zeros((3, 5)), np.ones((3, 5)), 0)
        assert a.shape == b.shape == (3, 5) and np.all(a == 1.0) and np.all(b == 2.0) and seen[-1] == (inverse, 15, 0)
        a, b = method(np.zeros(4, dtype=np.float32), np.ones(4, dtype=np.int64), 1)
        assert a.shape == b.shape == (4,) and a.dtype == np.float64
        a, b = method(3.0, 4, 0)
        assert np.ndim(a) == 0 and np.ndim(b) == 0 and (a, b) == (4.0, 5.0) and seen[-1] == (inverse, 1, 0)
        with pytest.raises(TypeError):
            method(np.zeros((2, 2)))
    assert w.array_shape == (4088, 4088) and w.constructortype == "FITSHEADER" and w.type == "ASTROPY"


def test_destripe_pair_takes_exactly_one_way():
    from pyimcom_amd import wcs as W
    from pyimcom_amd.destripe import DestripeEngine

    eng = DestripeEngine.__new__(DestripeEngine)
    eng.nside, eng._scas, eng._pairs, eng.L, eng._tables = 64, [None, None], {}, 0, None
    w = W.DeviceWCS.from_header(CASES["small_a"]["header"], array_shape=(64, 64))
    z = np.zeros((64, 64))
    for kw in (dict(x=z, y=z, wcs=(w, w)), dict(lattice=np.zeros((2, 5, 5)), wcs=(w, w)), dict(x=z, y=z, lattice=np.zeros((2, 5, 5))), dict(), dict(x=z)):
        with pytest.raises(ValueError):
            eng.set_pair(0, 1, **kw)
    with pytest.raises(ValueError):
        eng.set_pair(0, 1, wcs=(W.DeviceWCS.from_header(CASES["small_a"]["header"]), w))  # a 4088-pixel WCS for a 64-pixel engine
    eng.set_pair(0, 1, wcs=(w, CASES["small_b"]["header"]))
    assert eng._pairs[(0, 1)][0] == "wcs" and isinstance(eng._pairs[(0, 1)][2], W.DeviceWCS)


# ---- the core as a host program ---------------------------------------------------------------------------------------------------------

def _jobs_file(path):
    tab64, tab32 = G["table_f64"], G["table_f32"]
    parts = [np.array([tab64.shape[1], G["table_ends"][0], G["table_ends"][1]]), tab64.ravel(), tab32.astype(np.float64).ravel()]
    jobs = []
    kind_of = {None: 0, "f32": 1, "f64": 2}
    zero = np.zeros(R.DESC_LEN)
    for name, c in CASES.items():
        d, t = G[name + "_desc"], kind_of[c["table"]]
        for kind, src, dst, err in ((0, "_pix", "_world", "_world_err"), (1, "_world", "_inv", "_inv_err")):
            bound = 10 * G[name + err]
            jobs.append(np.concatenate(([kind, c["origin"], len(G[name + src]), bound[0], bound[1], t], d, [0], zero, G[name + src].ravel(), G[name + dst].ravel())))
    for p in META["pairs"]:
        a, b = CASES[p["from"]], CASES[p["to"]]
        bound = 10 * G[p["name"] + "_err"]
        pix = G[a["name"] + "_pix"]
        jobs.append(np.concatenate(([2, p["origin"], len(pix), bound[0], bound[1], kind_of[a["table"]]], G[a["name"] + "_desc"], [kind_of[b["table"]]],
                                    G[b["name"] + "_desc"], pix.ravel(), G[p["name"] + "_xy"].ravel())))
    parts.append(np.array([len(jobs)], dtype=np.float64))
    np.concatenate(parts + jobs).astype(np.float64).tofile(path)
    return sum(int(j[2]) for j in jobs)


def test_native_core_against_the_fixture_under_sanitizers(tmp_path):
    exe, jobs = tmp_path / "wcs_check", tmp_path / "jobs.bin"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "pyimcom_amd", "csrc"), os.path.join(ROOT, "tests", "native", "wcs_check.cpp"), "-o", str(exe)])
    npoints = _jobs_file(str(jobs))
    out = subprocess.run([str(exe), str(jobs)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.strip().splitlines()]
    assert [r[0] for r in rows] == ["fixture", "cells", "newton", "exits"]
    assert int(rows[0][1]) == npoints and int(rows[1][1]) > 150 and all(int(r[2]) == 0 for r in rows), rows


@pytest.mark.parametrize("name", ["imcom_wcs_pix2world", "imcom_wcs_world2pix", "imcom_wcs_pix2pix", "imcom_wcs_pix_area"])
def test_null_context_is_refused_before_anything_else(name):
    """Each of the seam's context-taking entries refuses a null context with every other argument zero."""
    import ctypes as C

    from pyimcom_amd import _lib

    def null(t):
        if t in (C.c_double, C.c_float):
            return 0.0
        return 0 if isinstance(t, type) and issubclass(t, C._SimpleCData) and t._type_ in "bBhHiIlLqQ" else None

    assert getattr(_lib.lib, name)(*[null(t) for t in _lib.SIGNATURES[name]]) == -1
    assert "null context" in _lib.lib.imcom_last_error().decode()
