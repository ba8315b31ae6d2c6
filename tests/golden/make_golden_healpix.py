"""Writes tests/golden/healpix.npz (seam 18).  The reference's own statements -- ``GridInject.make_sph_grid`` and ``generate_star_grid``
(src/pyimcom/layer.py:690-789), the statement block of ``StarsAnal.__call__`` (analysis.py:957-978) and the position angle of
``gen_truthcats`` (truthcats.py:229-241) -- are taken out of the syntax tree and executed with tests/healpix_reference.py standing in for
``healpy`` and tests/wcs_reference.py's numpy chain standing in for the WCS (layer.py cannot be imported here: galsim, healpy and astropy at
module level).  Recorded per case: the statements' outputs; the exact centres (mpmath, 40 digits, rounded to float64) of every recorded
pixel; ``ref_err``, the largest distance of the float64 restatement from them; and the smallest ``|mu_exact - cos r|`` over the candidates.

A case whose margin is below 1e-12 is refused: a float64 ``mu`` is off by a few 1e-16, so above the margin membership is the same for every
faithful evaluation.  A block case with an ``x`` or ``y`` within 1e-6 pixel of a half-integer at the box edge is refused as well.  healpy is
not installed where this runs: nothing here comes from healpy.  Run from the repository root:  python tests/golden/make_golden_healpix.py"""

import ast
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import healpix_reference as R  # noqa: E402
from tests import wcs_reference as RW  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "healpix.npz")
REF = "/root/reference/src/pyimcom/"
MARGIN, EDGE = 1e-12, 1e-6
NEAR = 1e-9  # candidates whose float64 mu is this close to cos r get the 40-digit mu (a float64 mu is off by a few 1e-16)
SCA_RADIUS = 4088 * 0.11 / 3600 * (np.pi / 180)

CAPS = [  # name, res, ra, dec, radius (radians)
    ("r5_a", 5, 0.001, 0.3, 0.2),
    ("r5_wrap", 5, 6.28, -0.2, 0.15),
    ("r5_north", 5, 1.0, 1.45, 0.2),
    ("r5_pole", 5, 2.0, -1.5, 0.12),  # the clipped pole: 42 of the disc's 44
    ("r5_edge", 5, 3.0, float(np.arcsin(2.0 / 3.0)), 0.1),  # the belt / cap transition
    ("r5_equator", 5, 0.5, 0.0, 0.05),
    ("r5_empty", 5, 0.7, 0.4, 0.004),  # smaller than a pixel and between centres: no hit
    ("r14_m30", 14, float(np.radians(50.0)), float(np.radians(-30.0)), SCA_RADIUS),
    ("r14_edge", 14, 1e-5, float(np.arcsin(2.0 / 3.0)), SCA_RADIUS),
    ("r14_m44", 14, float(np.radians(9.7)), float(np.radians(-44.1)), SCA_RADIUS),
    ("r14_wrap", 14, float(np.radians(359.999)), float(np.radians(5.0)), SCA_RADIUS),
]
STAR_GRID = {"wcs_case": "sip2_m40_b", "res": 13}  # a TAN-SIP header of tests/golden/wcs.npz
BLOCK = {"res": 10, "n": 200, "bdpad": 40, "search_radius": 0.0206,
         "header": {"CTYPE1": "RA---STG", "CTYPE2": "DEC--STG", "CRPIX1": 100.5, "CRPIX2": 100.5, "CRVAL1": 53.0, "CRVAL2": -40.0,
                    "CD1_1": -1.0 / 120.0, "CD1_2": 0.0, "CD2_1": 0.0, "CD2_2": 1.0 / 120.0}}


class NumpyWCS:
    """tests/wcs_reference.py's float64 chain with the call forms the reference's statements use."""

    def __init__(self, desc, pixel_n_dim=2):
        self.desc, self.pixel_n_dim = np.asarray(desc, dtype=np.float64), pixel_n_dim

    def all_pix2world(self, *args, **kw):
        if len(args) == 2:
            pos = np.array(args[0], dtype=np.float64).reshape(-1, 2)
            return np.stack(RW.np_pix2world(self.desc, None, pos[:, 0], pos[:, 1], args[1]), axis=1)
        x, y, origin = np.asarray(args[0], dtype=np.float64), np.asarray(args[1], dtype=np.float64), args[-1]
        return RW.np_pix2world(self.desc, None, x, y, origin)

    def all_world2pix(self, *args):
        ra, dec, origin = np.asarray(args[0], dtype=np.float64), np.asarray(args[1], dtype=np.float64), args[-1]
        x, y, ok = RW.np_world2pix(self.desc, None, ra, dec, origin)
        assert ok.all()
        return (x, y) if len(args) == 3 else (x, y, np.zeros_like(x), np.zeros_like(x))


def _statements(body, ranges):
    out = []
    for st in body:
        if any(lo <= st.lineno and st.end_lineno <= hi for lo, hi in ranges):
            out.append(st)
            continue
        for field in ("body", "orelse", "finalbody"):
            out += _statements(getattr(st, field, []) or [], ranges)
    return out


def reference_code():
    """GridInject with its two functions; the statement blocks of analysis.py and truthcats.py."""
    tree = ast.parse(open(REF + "layer.py").read(), filename="layer.py")
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "GridInject")
    cls.body = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in ("make_sph_grid", "generate_star_grid")]
    cls.bases = []
    ns = {"np": np, "healpy": R}
    exec(compile(ast.Module(body=[cls], type_ignores=[]), "layer.py", "exec"), ns)

    def block(path, func, ranges):
        t = ast.parse(open(REF + path).read(), filename=path)
        fn = next(n for n in ast.walk(t) if isinstance(n, ast.FunctionDef) and n.name == func and n.lineno <= ranges[0][0] <= n.end_lineno)
        return compile(ast.Module(body=_statements(fn.body, ranges), type_ignores=[]), path, "exec")

    return ns["GridInject"], block("analysis.py", "__call__", [(957, 978)]), block("truthcats.py", "gen_truthcats", [(229, 241)])


def exact_centres(nside, ipix):
    """(theta, phi) float64 [n] of the 40-digit centres, and ref_err [2] of the restatement."""
    th, ph = (np.array(v, dtype=object) for v in zip(*[R.mp_pix2ang(nside, p) for p in ipix])) if len(ipix) else (np.zeros(0, object), np.zeros(0, object))
    t64, p64 = R.pix2ang(nside, np.asarray(ipix, dtype=np.int64))
    err = [max((abs(a - float(b)) for a, b in zip(th, t64)), default=0.0), max((abs(a - float(b)) for a, b in zip(ph, p64)), default=0.0)]
    return np.array([float(v) for v in th]), np.array([float(v) for v in ph]), np.array([float(e) for e in err])


def cap_margin(nside, ra, dec, radius, pmin, pmax, chunk=1 << 22):
    """The smallest |mu_exact - cos r| over the candidates pmin .. pmax."""
    mp = R._mp()
    c, best = np.cos(radius), np.inf
    cexact = mp.cos(mp.mpf(float(radius)))
    for lo in range(int(pmin), int(pmax) + 1, chunk):
        p = np.arange(lo, min(lo + chunk, int(pmax) + 1), dtype=np.int64)
        d = np.abs(R.cap_mu(ra, dec, *R.pix2ang(nside, p)) - c)
        best = min(best, float(d[d >= NEAR].min()) if np.any(d >= NEAR) else np.inf)
        for q in p[d < NEAR]:
            best = min(best, float(abs(R.mp_cap_mu(ra, dec, *R.mp_pix2ang(nside, q)) - cexact)))
    return best


def res29_pixels():
    n = 1 << 29
    npix, ncap = 12 * n * n, 2 * n * (n - 1)
    p = [0, 1, 3, 4, ncap - 1, ncap, ncap + 4 * n - 1, ncap + 4 * n, npix - ncap - 4 * n, npix - ncap - 1, npix - ncap, npix - ncap + 1, npix - 1, npix - 4, npix - 5]
    for i in (2, 3, 1000, (1 << 28) + 1, n - 1):  # 1 + 2 p = (2 i - 1)^2 at the first pixel of ring i, and the mirror in the south
        s = 2 * i * (i - 1)
        assert math.isqrt(1 + 2 * s) ** 2 == 1 + 2 * s
        p += [s - 1, s, s + 1, npix - s - 1, npix - s, npix - s + 1]
    rng = np.random.default_rng(29)
    while len(set(p)) < 64:
        p.append(int(rng.integers(0, npix)))
    return np.array(sorted(set(p)), dtype=np.int64)


def mp_world2pix_exact(P, theta, phi, ddec_deg=0):
    """The 40-digit pixel position of the 40-digit centre (theta, phi), its declination moved by ddec_deg degrees."""
    mp = R._mp()
    delta = mp.pi / 2 - theta + mp.mpf(ddec_deg) * mp.pi / 180
    return RW.mp_native2pix(P, None, 0, *RW.mp_world2native(P, phi, delta), 0)


def positions(P, nside, ipix, want_pa=False):
    mp = R._mp()
    xy, pa = [], []
    for p in ipix:
        theta, phi = R.mp_pix2ang(nside, p)
        xy.append(mp_world2pix_exact(P, theta, phi))
        if want_pa:
            (xp, yp), (xm, ym) = mp_world2pix_exact(P, theta, phi, mp.mpf(1) / 3600), mp_world2pix_exact(P, theta, phi, -mp.mpf(1) / 3600)
            a = mp.atan2(xp - xm, yp - ym) * 180 / mp.pi
            pa.append(a - 360 * mp.floor(a / 360))
    return xy, pa


def compute():
    from pyimcom_amd import wcs as W

    GridInject, anal_code, pa_code = reference_code()
    out, meta = {}, {"caps": [], "margin": MARGIN, "edge": EDGE}

    sets = {"lowres": [(res, p) for res in range(4) for p in range(12 * 4 ** res)], "res29": [(29, int(p)) for p in res29_pixels()]}
    for name, pix in sets.items():
        res, ipix = np.array([r for r, _ in pix]), np.array([p for _, p in pix], dtype=np.int64)
        th, ph, err = np.zeros(len(pix)), np.zeros(len(pix)), np.zeros(2)
        for r in sorted(set(res.tolist())):
            m = res == r
            th[m], ph[m], e = exact_centres(1 << r, ipix[m])
            err = np.maximum(err, e)
        out[f"{name}_res"], out[f"{name}_ipix"], out[f"{name}_theta"], out[f"{name}_phi"], out[f"{name}_err"] = res, ipix, th, ph, err

    for name, res, ra, dec, radius in CAPS:
        nside = 1 << res
        g = GridInject.make_sph_grid(res, ra, dec, radius)
        pmin, pmax = R.reference_range(nside, ra, dec, radius)
        dlo, dhi = R.disc_range(nside, ra, dec, radius)
        margin = cap_margin(nside, ra, dec, radius, dlo, dhi)
        if margin < MARGIN:
            raise SystemExit(f"{name}: a candidate within {margin:.2e} of the circle; choose another case")
        disc = R.cap_brute(nside, ra, dec, radius, dlo, dhi)[0]
        assert set(g["ipix"]) <= set(disc) and g["npix"] == len(g["ipix"]) and np.all(np.diff(g["ipix"]) > 0)
        every = np.union1d(g["ipix"], disc)
        th, ph, err = exact_centres(nside, every)
        out[f"{name}_ipix"], out[f"{name}_rapix"], out[f"{name}_decpix"], out[f"{name}_disc"] = g["ipix"], g["rapix"], g["decpix"], disc
        out[f"{name}_theta"], out[f"{name}_phi"], out[f"{name}_err"] = th, ph, err
        meta["caps"].append({"name": name, "res": res, "ra": ra, "dec": dec, "radius": radius, "npix": int(g["npix"]), "ndisc": len(disc), "margin": margin,
                             "pmin": int(pmin), "pmax": int(pmax)})
        print(f"{name}: {g['npix']} pixels ({len(disc)} in the disc), margin {margin:.2e}, ref_err {err}", flush=True)

    # generate_star_grid on a TAN-SIP header
    GW = np.load(os.path.join(ROOT, "tests", "golden", "wcs.npz"))
    case = next(c for c in json.loads(str(GW["meta"]))["cases"] if c["name"] == STAR_GRID["wcs_case"])
    desc = GW[case["name"] + "_desc"]
    assert np.array_equal(desc, W.DeviceWCS.from_header(case["header"]).descriptor)
    res = STAR_GRID["res"]
    ipix, px, py, ra_deg, dec_deg = GridInject.generate_star_grid(res, NumpyWCS(desc))
    cen = NumpyWCS(desc).all_pix2world([[2043.5, 2043.5]], 0)[0] * (np.pi / 180)
    margin = cap_margin(1 << res, cen[0], cen[1], SCA_RADIUS, *R.reference_range(1 << res, cen[0], cen[1], SCA_RADIUS))
    if margin < MARGIN:
        raise SystemExit(f"star grid: margin {margin:.2e}")
    xy, _ = positions(RW.header_params(case["header"]), 1 << res, ipix)
    out["grid_ipix"], out["grid_px"], out["grid_py"], out["grid_ra"], out["grid_dec"] = ipix, px, py, ra_deg, dec_deg
    out["grid_xy"] = np.array([[float(x), float(y)] for x, y in xy])
    out["grid_err"] = np.array([float(max(abs(x - a) for (x, _), a in zip(xy, px))), float(max(abs(y - b) for (_, y), b in zip(xy, py)))])
    meta["grid"] = dict(STAR_GRID, header=case["header"], npix=len(ipix), margin=margin, centre=[float(cen[0]), float(cen[1])])
    print(f"star grid: {len(ipix)} pixels, margin {margin:.2e}, ref_err {out['grid_err']}", flush=True)

    # the block grid of the report sites, with the position angle
    b = BLOCK
    desc = W.DeviceWCS.from_header(b["header"], array_shape=(b["n"], b["n"])).descriptor
    ns = {"np": np, "numpy": np, "healpy": R, "mywcs": NumpyWCS(desc), "n": b["n"], "res": b["res"], "search_radius": b["search_radius"], "bdpad": b["bdpad"]}
    exec(anal_code, ns)
    ipix, nside = ns["qp"][ns["grp"]], 1 << b["res"]
    theta_c, phi_c = R.vec2ang(ns["vec"])
    ra_c, dec_c = float(phi_c[0]), float(np.pi / 2.0 - theta_c[0])
    margin = cap_margin(nside, ra_c, dec_c, b["search_radius"], *R.disc_range(nside, ra_c, dec_c, b["search_radius"]))
    xa, ya = NumpyWCS(desc).all_world2pix(*R.pix2ang(nside, ns["qp"], lonlat=True), 0)
    edge = min(float(np.min(np.abs(v - e))) for v in (xa, ya) for e in (b["bdpad"] - 0.5, b["n"] - b["bdpad"] - 0.5))
    if margin < MARGIN or edge < EDGE:
        raise SystemExit(f"block grid: margin {margin:.2e}, distance from the box edge {edge:.2e}")
    exec(pa_code, ns)
    xy, pa = positions(RW.header_params(b["header"]), nside, ipix, want_pa=True)
    for k in ("x", "y", "xi", "yi", "ra_hpix", "dec_hpix", "pa_hpix"):
        out["block_" + k.replace("_hpix", "")] = ns[k]
    out["block_ipix"], out["block_disc"] = ipix, ns["qp"]
    out["block_xy"], out["block_pa_exact"] = np.array([[float(x), float(y)] for x, y in xy]), np.array([float(a) for a in pa])
    dpa = [abs(a - float(v)) for a, v in zip(pa, ns["pa_hpix"])]
    out["block_err"] = np.array([float(max(abs(x - a) for (x, _), a in zip(xy, ns["x"]))), float(max(abs(y - a) for (_, y), a in zip(xy, ns["y"]))),
                                 float(max(min(d, 360 - d) for d in dpa))])
    meta["block"] = dict(b, npix=len(ipix), ndisc=len(ns["qp"]), margin=margin, edge=edge, centre=[ra_c, dec_c])
    print(f"block grid: {len(ipix)} of {len(ns['qp'])} pixels, margin {margin:.2e}, edge {edge:.2e}, ref_err {out['block_err']}", flush=True)
    out["meta"] = np.array(json.dumps(meta))
    return out


if __name__ == "__main__":
    np.savez_compressed(OUT, **compute())
    print(OUT, os.path.getsize(OUT), "bytes")
