"""Writes tests/golden/wcs.npz (seam 16): the cases' headers, packed descriptors and points, the results of the published definitions in
40-digit arithmetic rounded to float64 (tests/wcs_reference.py, mpmath), and per case and quantity ``ref_err``: the largest distance of the
float64 numpy restatement from them.  astropy is not installed where this runs: nothing here comes from astropy or from the reference's own
run.  Run from the repository root:  python tests/golden/make_golden_wcs.py [--check K]   (--check: recompute the first K points of every
case and compare with the file instead of writing it)."""

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import wcs_reference as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "wcs.npz")
ASEC = 1.0 / 3600.0
S = 0.11 * ASEC  # the Roman pixel scale in degrees


def _rot(scale, angle_deg, flip):
    c, s = np.cos(np.deg2rad(angle_deg)), np.sin(np.deg2rad(angle_deg))
    return {"CD1_1": float(-scale * c * flip), "CD1_2": float(scale * s), "CD2_1": float(scale * s * flip), "CD2_2": float(scale * c)}


def _sip(order_a, order_b, seed, half):
    """Coefficients whose terms reach a few pixels at the chip's edge (|u| = half)."""
    rng = np.random.default_rng(seed)
    h = {}
    for L, order in (("A", order_a), ("B", order_b)):
        if order:
            h[f"{L}_ORDER"] = order
        for p in range(order + 1):
            for q in range(order + 1 - p):
                if p + q >= 2:
                    h[f"{L}_{p}_{q}"] = float(rng.uniform(-1, 1) * 2.0 / half ** (p + q) / (p + q - 1))
    return h


def _header(proj, ra, dec, cd, crpix, sip=None, lonpole=None):
    h = {"CTYPE1": "RA---" + proj, "CTYPE2": "DEC--" + proj, "CRPIX1": crpix, "CRPIX2": crpix, "CRVAL1": ra, "CRVAL2": dec}
    h.update(cd)
    if lonpole is not None:
        h["LONPOLE"] = lonpole
    h.update(sip or {})
    return h


BIG, SMALL, TINY = 4088, 250, 48
CASES = [
    # name, header, nside, origin, table kind, niter
    ("tan_m40", _header("TAN", 53.1, -40.0, _rot(S, 31.0, 1), 2044.5), BIG, 0, None, 0),
    ("sip2_m40", _header("TAN-SIP", 53.1, -40.0, _rot(S, -12.0, -1), 2044.5, _sip(2, 2, 1, 2044.0)), BIG, 1, None, 0),
    ("sip2_m40_b", _header("TAN-SIP", 53.16, -40.03, _rot(S, 47.0, 1), 2044.5, _sip(2, 2, 2, 2044.0)), BIG, 0, None, 0),
    ("sip4_wrap", _header("TAN-SIP", 359.99, 12.0, _rot(S, 75.0, 1), 2044.5, _sip(4, 3, 3, 2044.0), lonpole=137.0), BIG, 0, None, 0),
    ("sip4_wrap_b", _header("TAN-SIP", 0.01, 12.02, _rot(S, 160.0, -1), 2044.5, _sip(3, 4, 4, 2044.0)), BIG, 1, None, 0),
    ("sip2_pole", _header("TAN-SIP", 201.0, 89.9, _rot(S, 5.0, 1), 2044.5, _sip(2, 2, 5, 2044.0)), BIG, 0, None, 0),
    ("sip2_pole_b", _header("TAN-SIP", 215.0, 89.93, _rot(S, -100.0, 1), 2044.5, _sip(2, 2, 6, 2044.0), lonpole=137.0), BIG, 0, None, 0),
    ("stg_pole", _header("STG", 10.0, 89.9, _rot(0.39 * ASEC, 0.0, 1), 2044.5), BIG, 0, None, 0),  # the pole is 923 pixels from CRPIX
    ("stg_m40", _header("STG", 53.12, -40.01, _rot(0.0390625 * ASEC, 20.0, 1), 2044.5, lonpole=137.0), BIG, 1, None, 0),
    ("small_a", _header("TAN-SIP", 150.0, 2.2, _rot(S, 10.0, 1), 125.5, _sip(2, 2, 7, 125.0)), SMALL, 0, None, 0),
    ("small_b", _header("TAN-SIP", 150.004, 2.203, _rot(S, 33.0, -1), 125.5, _sip(3, 2, 8, 125.0)), SMALL, 0, None, 0),
    ("small_c", _header("TAN", 150.006, 2.197, _rot(S, -50.0, 1), 125.5), SMALL, 0, None, 0),
    ("small_d", _header("TAN-SIP", 150.3, 2.2, _rot(S, 0.0, 1), 125.5, _sip(2, 2, 9, 125.0)), SMALL, 0, None, 0),    # disjoint from a, b, c
    ("small_e", _header("TAN", 359.999, -0.2, _rot(S, 0.0, 1), 125.5), SMALL, 0, None, 0),                            # and so is this
    ("tab32_n3", _header("TAN-SIP", 80.0, -30.0, _rot(S, 15.0, 1), 24.5, _sip(2, 2, 10, 100.0)), TINY, 0, "f32", 3),
    ("tab64_n1", _header("TAN-SIP", 80.0, -30.0, _rot(S, 15.0, 1), 24.5, _sip(2, 2, 10, 100.0)), TINY, 1, "f64", 1),
    ("tab64_n0", _header("TAN-SIP", 80.0, -30.0, _rot(S, 15.0, -1), 24.5, _sip(2, 2, 11, 100.0)), TINY, 0, "f64", 0),
]
# name, from, to: the first three are the Roman-scale TAN-SIP -> TAN-SIP chains whose ref_err the issue of the seam bounds
PAIRS = [("chain_m40", "sip2_m40", "sip2_m40_b"), ("chain_pole", "sip2_pole", "sip2_pole_b"), ("chain_wrap", "sip4_wrap", "sip4_wrap_b"),
         ("to_stg", "sip2_m40_b", "stg_m40"), ("from_stg", "stg_pole", "sip2_pole"), ("plain", "tan_m40", "sip2_m40"), ("tab_chain", "tab32_n3", "tab64_n1"),
         ("tab_chain0", "tab64_n1", "tab64_n0")]
GRID = ("small_a", "small_b", 3, 7)  # map_sca2sca(target, ref, pad, subsamp): 37 x 37 points, a subset of the subsamp = 1 grid
AREAS = [("area_plain", "small_b", [100, 112, 40, 50], 1, 1), ("area_wrap", "small_e", [86, 98, 60, 68], 2, 1)]  # the second straddles ra = 0
NPTS = {BIG: 1100, SMALL: 300, TINY: 500}
TAB_A, TAB_NPAD = 8, 24


def errmap(n=TINY):
    """A smooth map of a few hundredths of a pixel plus small-scale structure, [2, n, n] float64."""
    rng = np.random.default_rng(77)
    y, x = np.mgrid[0:n, 0:n] / float(n)
    m = np.stack((0.04 * np.sin(3.1 * x + 1.3 * y) + 0.01 * x * y, 0.03 * np.cos(2.2 * y - 0.7 * x) - 0.02 * y * y))
    return m + 2e-3 * rng.standard_normal(m.shape)


def tables():
    """{kind: (values [2, N + 2, N + 2], lo, hi)}: the padded grid of LocWCS.err_interp on the raw map (pyimcom_amd.wcs.error_table;
    tests/test_wcs_host.py holds it to its definition and scipy's interpolator on it to the restatement)."""
    from pyimcom_amd import wcs as W

    return {kind: W.error_table(errmap(), a=TAB_A, n_pad=TAB_NPAD, use_float32=kind == "f32") for kind in ("f32", "f64")}


def points(name, nside, header):
    """[n, 2]: CRPIX itself (r = 0, in the case's origin it is appended by the caller), the corners 50 pixels off the chip, then uniform
    draws over the chip and 50 pixels around it (the tiny chips: beyond both ends of the table)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    m = 50.0 if nside != TINY else 70.0
    lo, hi = -m, nside - 1 + m
    fixed = [[lo, lo], [lo, hi], [hi, lo], [hi, hi], [0.0, 0.0], [nside - 1.0, nside - 1.0], [-0.5, nside - 0.5]]
    if nside == TINY:
        fixed += [[float(k), float(k)] for k in range(0, TINY)] + [[-24.0, 71.0], [-30.0, 80.0], [-10.5, 60.25], [47.0, 46.999]]
    p = np.vstack((np.array(fixed), rng.uniform(lo, hi, size=(NPTS[nside] - len(fixed) - 1, 2))))
    return p


def pack(header, nside, table, niter):
    from pyimcom_amd import wcs as W

    return W.DeviceWCS.from_header(header, array_shape=(nside, nside), table=table, niter=niter).descriptor


def compute(limit=None):
    out = {}
    tabs = tables()
    for kind, (t, lo, hi) in tabs.items():
        out[f"table_{kind}"] = t
    out["table_ends"] = np.array([tabs["f64"][1], tabs["f64"][2]])
    out["errmap"] = errmap()
    meta = {"cases": [], "pairs": [], "areas": [], "grid": None, "tab_a": TAB_A, "tab_npad": TAB_NPAD}
    cases = {}
    for name, header, nside, origin, kind, niter in CASES:
        tab = tabs[kind] if kind else None
        desc = pack(header, nside, tab, niter)
        P = R.header_params(header)
        crpix_pt = np.array([[header["CRPIX1"] - 1 + origin, header["CRPIX2"] - 1 + origin]])
        pix = np.vstack((crpix_pt, points(name, nside, header)))
        if limit:
            pix = pix[:limit]
        cases[name] = (header, nside, origin, kind, niter, desc, P, tab, pix)
        meta["cases"].append({"name": name, "header": header, "nside": nside, "origin": origin, "table": kind, "niter": niter})
        # forward
        ex = [R.mp_pix2world(P, tab, x, y, origin) for x, y in pix]
        ra, dec = R.np_pix2world(desc, tab, pix[:, 0], pix[:, 1], origin)
        world = np.array([[float(a), float(d)] for a, d in ex])
        werr = [max(float(min(abs(a - float(r)), 360 - abs(a - float(r)))) for (a, _), r in zip(ex, ra)), max(float(abs(d - float(v))) for (_, d), v in zip(ex, dec))]
        # inverse, from the rounded world coordinates
        inv = [R.mp_world2pix(P, tab, niter, a, d, origin) for a, d in world]
        xn, yn, ok = R.np_world2pix(desc, tab, world[:, 0], world[:, 1], origin)
        assert ok.all(), name
        ierr = [max(float(abs(e[0] - float(v))) for e, v in zip(inv, xn)), max(float(abs(e[1] - float(v))) for e, v in zip(inv, yn))]
        out[f"{name}_desc"], out[f"{name}_pix"], out[f"{name}_world"] = desc, pix, world
        out[f"{name}_inv"] = np.array([[float(a), float(b)] for a, b in inv])
        out[f"{name}_world_err"], out[f"{name}_inv_err"] = np.array(werr), np.array(ierr)
        print(f"{name:12s} n={len(pix):5d} world ref_err {werr[0]:.2e} {werr[1]:.2e} deg   inverse ref_err {ierr[0]:.2e} {ierr[1]:.2e} pixel"
              f"   round trip {np.nanmax(np.abs(np.stack((xn, yn), 1) - pix)):.2e}", flush=True)

    def chain(label, a, b, pix, origin):
        ha, _, _, _, _, da, Pa, ta, _ = cases[a]
        hb, _, _, _, nb, db, Pb, tb, _ = cases[b]
        ex = [R.mp_pix2pix(Pa, ta, Pb, tb, nb, x, y, origin) for x, y in pix]
        xn, yn, ok = R.np_pix2pix(da, ta, db, tb, pix[:, 0], pix[:, 1], origin)
        assert ok.all(), label
        err = [max(float(abs(e[0] - float(v))) for e, v in zip(ex, xn)), max(float(abs(e[1] - float(v))) for e, v in zip(ex, yn))]
        print(f"{label:12s} n={len(pix):5d} pix2pix ref_err {err[0]:.2e} {err[1]:.2e} pixel", flush=True)
        return np.array([[float(p), float(q)] for p, q in ex]), np.array(err)

    for label, a, b in PAIRS:
        origin = cases[a][2]
        out[f"{label}_xy"], out[f"{label}_err"] = chain(label, a, b, cases[a][8], origin)
        meta["pairs"].append({"name": label, "from": a, "to": b, "origin": origin})
    a, b, pad, sub = GRID
    s = R.grid_axis(cases[a][1], pad, sub)
    gx, gy = np.meshgrid(s, s)
    gp = np.stack((gx.ravel(), gy.ravel()), 1)
    if limit:
        gp = gp[:limit]
    out["grid_xy"], out["grid_err"] = chain("grid", a, b, gp, 0)
    meta["grid"] = {"target": a, "ref": b, "pad": pad, "subsamp": sub}
    for label, c, region, pad, ovsamp in AREAS:
        header, nside, origin, kind, niter, desc, P, tab, _ = cases[c]
        if limit:
            region = [region[0], region[0] + 2, region[2], region[2] + 2]
        ex = R.mp_pix_area(P, tab, region, pad, ovsamp)
        got, turned = R.np_pix_area(desc, tab, region, pad, ovsamp)
        out[f"{label}_area"], out[f"{label}_err"] = ex, np.array([np.max(np.abs(got - ex))])
        meta["areas"].append({"name": label, "case": c, "region": region, "pad": pad, "ovsamp": ovsamp, "turned": turned})
        print(f"{label:12s} {ex.shape} area ref_err {out[label + '_err'][0]:.2e} of {ex.mean():.3e} square degrees, turned: {turned}", flush=True)
    out["meta"] = np.array(json.dumps(meta))
    return out


if __name__ == "__main__":
    if "--check" in sys.argv:
        k = int(sys.argv[sys.argv.index("--check") + 1])
        new, old = compute(limit=k), np.load(OUT)
        for key, v in new.items():
            if key.endswith(("_world", "_inv", "_xy")):
                assert np.array_equal(v, old[key][:len(v)]), key
        print("the first", k, "points of every case agree with", OUT)
    else:
        np.savez_compressed(OUT, **compute())
        print("wrote", OUT, os.path.getsize(OUT), "bytes")
