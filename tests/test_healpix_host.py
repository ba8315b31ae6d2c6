"""CPU-side checks of the device HEALPix grids (seam 18): the float64 numpy restatement that the device tests lean on
(tests/healpix_reference.py) against the 40-digit fixture; the round trip of every pixel of the low resolutions; the fixture regenerated; the
ring-window form of the cap against the brute force; csrc/healpix_core.h as a host program under the sanitizers; the refusals and the public
signatures.  healpy is not installed here: only the last test compares with healpy, where it is."""

import inspect
import json
import os
import subprocess

import numpy as np
import pytest

from tests import healpix_reference as R
from tests.conftest import ROOT

G = np.load(os.path.join(ROOT, "tests", "golden", "healpix.npz"))
META = json.loads(str(G["meta"]))
CAPS = {c["name"]: c for c in META["caps"]}


def angle_bound(err):
    """This project's bound for a device against a 40-digit value (seams 7, 9, 16): ten times the restatement's own distance, and not below
    four units in the last place of 2 pi."""
    return np.maximum(10 * np.asarray(err), R.ANGLE_FLOOR)


def seeded_caps():
    rng = np.random.default_rng(18)
    return [(rng.uniform(0, 2 * np.pi), np.arcsin(rng.uniform(-1, 1)), rng.uniform(0.01, 0.6)) for _ in range(200)]


@pytest.mark.parametrize("name", ["lowres", "res29"] + sorted(CAPS))
def test_restatement_against_the_exact_centres(name):
    if name in CAPS:
        nside, ipix = 1 << CAPS[name]["res"], np.union1d(G[name + "_ipix"], G[name + "_disc"])
        theta, phi = R.pix2ang(nside, ipix) if ipix.size else (np.zeros(0), np.zeros(0))
    else:
        theta, phi = (np.array([R.pix2ang(1 << r, p)[k] for r, p in zip(G[name + "_res"], G[name + "_ipix"])]) for k in (0, 1))
    bt, bp = angle_bound(G[name + "_err"])
    assert np.all(np.abs(theta - G[name + "_theta"]) <= bt) and np.all(np.abs(phi - G[name + "_phi"]) <= bp)
    assert np.all(G[name + "_err"] < 2e-15)  # (a loose ref_err would hide a failure of the device)
    assert np.all((phi >= 0) & (phi < 2 * np.pi)) and np.all((theta > 0) & (theta < np.pi))


def test_sets_of_the_fixture_are_the_ones_the_issue_lists():
    assert [int(np.sum(G["lowres_res"] == r)) for r in range(4)] == [12, 48, 192, 768]
    n = 1 << 29
    p = set(G["res29_ipix"].tolist())
    assert len(p) == 64 and {0, 2 * n * (n - 1) - 1, 2 * n * (n - 1), 12 * n * n - 2 * n * (n - 1), 12 * n * n - 1, 4, 3, 5} <= p
    assert CAPS["r5_pole"]["npix"] == 42 and CAPS["r5_pole"]["ndisc"] == 44 and CAPS["r5_empty"]["npix"] == 0
    assert min(c["margin"] for c in CAPS.values()) >= META["margin"] and META["grid"]["margin"] >= META["margin"] and META["block"]["margin"] >= META["margin"]
    assert META["block"]["edge"] >= META["edge"]


@pytest.mark.parametrize("res", range(5))
def test_ang2pix_inverts_pix2ang_for_every_pixel(res):
    p = np.arange(12 * 4 ** res)
    theta, phi = R.pix2ang(1 << res, p)
    assert np.array_equal(R.ang2pix(1 << res, theta, phi), p)
    assert np.array_equal(R.ang2pix(1 << res, *R.pix2ang(1 << res, p, lonlat=True), lonlat=True), p)
    assert np.array_equal(R.ang2pix(1 << res, theta, phi - 4 * np.pi), p)


@pytest.mark.parametrize("name", [n for n in sorted(CAPS) if n.startswith("r5")] + ["r14_edge"])
def test_fixture_regenerates(name):
    """What the reference's statements gave is what the restatement gives, bit for bit (they ran with it as their healpy); the exact
    centres are recomputed where mpmath is installed."""
    c = CAPS[name]
    nside = 1 << c["res"]
    assert R.reference_range(nside, c["ra"], c["dec"], c["radius"]) == (c["pmin"], c["pmax"])
    ipix, theta, phi, _ = R.cap_brute(nside, c["ra"], c["dec"], c["radius"], c["pmin"], c["pmax"])
    assert np.array_equal(ipix, G[name + "_ipix"]) and np.array_equal(phi, G[name + "_rapix"]) and np.array_equal(np.pi / 2.0 - theta, G[name + "_decpix"])
    assert np.array_equal(R.cap_windowed(nside, c["ra"], c["dec"], c["radius"], full_disc=True)[0], G[name + "_disc"])
    if c["res"] == 5:  # (every pixel of the sphere)
        assert np.array_equal(np.nonzero(R.cap_mu(c["ra"], c["dec"], *R.pix2ang(nside, np.arange(12288))) >= np.cos(c["radius"]))[0], G[name + "_disc"])
    pytest.importorskip("mpmath")
    every = np.union1d(G[name + "_ipix"], G[name + "_disc"])
    for k in sorted({0, len(every) // 3, len(every) - 1} & set(range(len(every)))):
        t, p = R.mp_pix2ang(nside, every[k])
        assert (float(t), float(p)) == (G[name + "_theta"][k], G[name + "_phi"][k])


def test_exact_centres_of_res_29_regenerate():
    pytest.importorskip("mpmath")
    for k in range(0, 64, 7):
        t, p = R.mp_pix2ang(1 << 29, G["res29_ipix"][k])
        assert (float(t), float(p)) == (G["res29_theta"][k], G["res29_phi"][k])


def test_window_form_equals_brute_force_for_the_seeded_caps():
    theta, phi = R.pix2ang(64, np.arange(49152))
    hits = []
    for ra, dec, radius in seeded_caps():
        mu = R.cap_mu(ra, dec, theta, phi)
        assert np.min(np.abs(mu - np.cos(radius))) > 1e-9  # (far above what two float64 evaluations can differ by)
        brute = np.nonzero(mu >= np.cos(radius))[0]
        got, _, _, tested = R.cap_windowed(64, ra, dec, radius, full_disc=True)
        assert np.array_equal(got, brute)
        assert tested < 49152
        hits.append(brute.size)
    assert min(hits) >= 1 and max(hits) > 4000


# ---- the core as a host program ---------------------------------------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _jobs_file(path):
    jobs, ncaps, npix = [], 0, 0
    for name in ("lowres", "res29"):
        n = len(G[name + "_ipix"])
        rows = np.stack((G[name + "_res"].astype(np.int64), G[name + "_ipix"], _bits(G[name + "_theta"]), _bits(G[name + "_phi"])), axis=1)
        jobs.append(np.concatenate(([0, n], _bits(angle_bound(G[name + "_err"])), rows.ravel())))
        npix += n
    caps = [(c["res"], c["ra"], c["dec"], c["radius"], G[c["name"] + "_ipix"], G[c["name"] + "_disc"]) for c in META["caps"]]
    g, b = META["grid"], META["block"]
    caps.append((g["res"], g["centre"][0], g["centre"][1], 4088 * 0.11 / 3600 * (np.pi / 180), G["grid_ipix"], None))
    caps.append((b["res"], b["centre"][0], b["centre"][1], b["search_radius"], None, G["block_disc"]))
    for res, ra, dec, radius, ref, disc in caps:
        for mode, want in ((0, ref), (1, disc)):
            if want is not None:
                jobs.append(np.concatenate(([1, res], _bits([ra, dec, radius]), [mode, len(want)], want)).astype(np.int64))
                ncaps += 1
    np.concatenate([np.array([len(jobs)], dtype=np.int64)] + [np.asarray(j, dtype=np.int64) for j in jobs]).tofile(path)
    return npix, ncaps


def test_native_core_against_the_fixture_under_sanitizers(tmp_path):
    exe, jobs = tmp_path / "healpix_check", tmp_path / "jobs.bin"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "pyimcom_amd", "csrc"), os.path.join(ROOT, "tests", "native", "healpix_check.cpp"), "-o", str(exe)])
    npix, ncaps = _jobs_file(str(jobs))
    out = subprocess.run([str(exe), str(jobs)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.strip().splitlines()]
    assert [r[0] for r in rows] == ["pixels", "caps", "integers", "windows", "box"]
    assert int(rows[0][1]) == npix and int(rows[1][1]) == ncaps and all(int(r[2]) == 0 and int(r[1]) > 0 for r in rows), rows


# ---- the boundary -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["imcom_healpix_pix2ang", "imcom_healpix_ang2pix", "imcom_healpix_cap"])
def test_null_context_is_refused_before_anything_else(name):
    import ctypes as C

    from pyimcom_amd import _lib

    def null(t):
        if t in (C.c_double, C.c_float):
            return 0.0
        return 0 if isinstance(t, type) and issubclass(t, C._SimpleCData) and t._type_ in "bBhHiIlLqQ" else None

    assert getattr(_lib.lib, name)(*[null(t) for t in _lib.SIGNATURES[name]]) == -1
    assert "null context" in _lib.lib.imcom_last_error().decode()


def test_public_signatures_are_healpys_and_the_references():
    from pyimcom_amd import healpix as H

    def leading(fn, k):
        return [(p.name, p.default) for p in list(inspect.signature(fn).parameters.values())[:k]]

    E = inspect.Parameter.empty
    assert leading(H.pix2ang, 4) == [("nside", E), ("ipix", E), ("nest", False), ("lonlat", False)]
    assert leading(H.ang2pix, 5) == [("nside", E), ("theta", E), ("phi", E), ("nest", False), ("lonlat", False)]
    assert leading(H.ang2vec, 3) == [("theta", E), ("phi", E), ("lonlat", False)]
    assert leading(H.vec2ang, 2) == [("vectors", E), ("lonlat", False)]
    assert leading(H.query_disc, 5) == [("nside", E), ("vec", E), ("radius", E), ("inclusive", False), ("nest", False)]
    assert leading(H.make_sph_grid, 4) == [("res", E), ("ra", E), ("dec", E), ("radius", E)]
    assert leading(H.generate_star_grid, 3) == [("res", E), ("myWCS", E), ("scapar", {"nside": 4088, "pix_arcsec": 0.11})]
    assert leading(H.block_star_grid, 7) == [("res", E), ("wcs", E), ("n", E), ("bdpad", E), ("search_radius", E), ("position_angle", False), ("device_out", False)]
    # everything past the reference's parameters has a default: the functions can be passed where the reference's are expected
    for fn, k in ((H.pix2ang, 2), (H.ang2pix, 3), (H.query_disc, 3), (H.make_sph_grid, 4), (H.generate_star_grid, 2), (H.block_star_grid, 5)):
        assert all(p.default is not E for p in list(inspect.signature(fn).parameters.values())[k:])


def test_what_is_not_served_is_refused_as_unsupported():
    from pyimcom_amd import healpix as H
    from pyimcom_amd._lib import ImcomError

    for call in (lambda: H.pix2ang(4, [0], nest=True), lambda: H.ang2pix(4, 0.1, 0.2, nest=True), lambda: H.query_disc(4, [0, 0, 1], 0.1, nest=True),
                 lambda: H.query_disc(4, [0, 0, 1], 0.1, inclusive=True), lambda: H.pix2ang(12, [0]), lambda: H.pix2ang(1 << 30, [0])):
        with pytest.raises(ImcomError) as e:
            call()
        assert e.value.status == -4


def test_host_vectors_against_the_restatement():
    from pyimcom_amd import healpix as H

    rng = np.random.default_rng(3)
    theta, phi = np.arccos(rng.uniform(-1, 1, 50)), rng.uniform(0, 2 * np.pi, 50)
    v = H.ang2vec(theta, phi)
    assert np.array_equal(v, R.ang2vec(theta, phi)) and np.allclose(np.sum(v * v, axis=1), 1.0, atol=1e-15)
    t2, p2 = H.vec2ang(v)
    assert np.max(np.abs(t2 - theta)) < 1e-15 and np.max(np.abs(p2 - phi)) < 2e-15
    lon, lat = H.vec2ang(H.ang2vec(30.0, -45.0, lonlat=True), lonlat=True)
    assert abs(lon[0] - 30.0) < 1e-13 and abs(lat[0] + 45.0) < 1e-13


def test_against_healpy_where_it_is_installed():
    healpy = pytest.importorskip("healpy")
    for res in (0, 1, 5, 12):
        nside = 1 << res
        p = np.unique(np.concatenate((np.arange(min(12 * nside * nside, 3000)), np.random.default_rng(res).integers(0, 12 * nside * nside, 3000))))
        theta, phi = healpy.pix2ang(nside, p)
        t2, p2 = R.pix2ang(nside, p)
        assert np.max(np.abs(theta - t2)) < 4e-15 and np.max(np.abs(phi - p2)) < 4e-15
        assert np.array_equal(healpy.ang2pix(nside, theta, phi), R.ang2pix(nside, theta, phi))
    for c in CAPS.values():
        if c["res"] == 5:
            vec = healpy.ang2vec(np.pi / 2 - c["dec"], c["ra"])
            assert np.array_equal(healpy.query_disc(32, vec, c["radius"]), G[c["name"] + "_disc"])
