"""The device HEALPix grids (seam 18) on the GPU: pyimcom_amd.healpix against tests/golden/healpix.npz.  Integers, sets and counts are
compared with ``==``; angles with |device - exact| <= max(10 ref_err, 3.6e-15 rad) (ref_err: the float64 numpy restatement's own distance from
the 40-digit value, capped in tests/test_healpix_host.py; the floor is four units in the last place of 2 pi); positions with seam 16's
bound, ten times the restatement's distance from the 40-digit chain.  Every cap of the fixture keeps its candidates at least 1e-12 from
the circle (tests/golden/make_golden_healpix.py refuses the others), so membership is the same for every faithful float64 evaluation."""

import json
import os

import numpy as np
import pytest

from tests import healpix_reference as R
from tests.conftest import ROOT
from tests.test_healpix_host import angle_bound, seeded_caps

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(ROOT, "tests", "golden", "healpix.npz"))
META = json.loads(str(G["meta"]))
CAPS = {c["name"]: c for c in META["caps"]}


def report(label, err, bound):
    print(f"{label}: largest error {np.max(err, initial=0.0):.3e}, bound {bound:.3e}, ratio {np.max(err, initial=0.0) / bound:.3f}")


def grid_wcs():
    from pyimcom_amd import wcs as W

    return W.DeviceWCS.from_header(META["grid"]["header"])


def block_wcs():
    from pyimcom_amd import wcs as W

    b = META["block"]
    return W.DeviceWCS.from_header(b["header"], array_shape=(b["n"], b["n"]))


@pytest.mark.parametrize("name", ["lowres", "res29"])
def test_pix2ang_and_ang2pix_against_the_exact_centres(name):
    from pyimcom_amd import healpix as H

    res, ipix = G[name + "_res"], G[name + "_ipix"]
    bt, bp = angle_bound(G[name + "_err"])
    worst = np.zeros(2)
    for r in sorted(set(res.tolist())):
        m = res == r
        nside, p, et, ep = 1 << r, ipix[m], G[name + "_theta"][m], G[name + "_phi"][m]
        theta, phi = H.pix2ang(nside, p)
        assert isinstance(theta, np.ndarray) and theta.dtype == np.float64 and theta.shape == p.shape
        worst = np.maximum(worst, [np.max(np.abs(theta - et)), np.max(np.abs(phi - ep))])
        assert np.all(np.abs(theta - et) <= bt) and np.all(np.abs(phi - ep) <= bp), (r, worst / [bt, bp])
        assert np.all((phi >= 0) & (phi < 2 * np.pi))
        lon, lat = H.pix2ang(nside, p, lonlat=True)
        assert np.array_equal(lon, np.degrees(phi)) and np.array_equal(lat, 90.0 - np.degrees(theta))
        # the inverse: from the device's own centres, from the exact ones, with phi a few turns off, and in degrees
        for t, f in ((theta, phi), (et, ep), (theta, phi - 4 * np.pi), (theta, phi + 2 * np.pi)):
            got = H.ang2pix(nside, t, f)
            assert got.dtype == np.int64 and np.array_equal(got, p), r
        assert np.array_equal(H.ang2pix(nside, lon, lat, lonlat=True), p)
        assert np.array_equal(R.ang2pix(nside, theta, phi), p)
    report(f"{name} theta", worst[0], float(bt)), report(f"{name} phi", worst[1], float(bp))
    assert H.pix2ang(4, 7)[0].shape == () and int(H.ang2pix(4, *H.pix2ang(4, 7))) == 7  # scalars in, scalars out


def test_list_entries_refuse_what_is_outside():
    from pyimcom_amd import healpix as H
    from pyimcom_amd._lib import ImcomError

    for call in (lambda: H.pix2ang(4, [0, 192]), lambda: H.pix2ang(4, [-1]), lambda: H.ang2pix(4, [0.1, np.nan], [0.2, 0.3]), lambda: H.ang2pix(4, [0.1], [np.inf]),
                 lambda: H.ang2pix(4, [3.2], [0.0]), lambda: H.make_sph_grid(5, 0.1, 1.6, 0.1), lambda: H.make_sph_grid(5, 0.1, 0.2, -0.1)):
        with pytest.raises(ImcomError) as e:
            call()
        assert e.value.status == -1
    assert H.pix2ang(4, np.zeros(0, dtype=np.int64))[0].shape == (0,)
    assert H.pix2ang(4, [191])[0].shape == (1,)  # the last pixel is inside


@pytest.mark.parametrize("name", sorted(CAPS))
def test_make_sph_grid_and_query_disc_against_the_fixture(name):
    from pyimcom_amd import healpix as H

    c = CAPS[name]
    g = H.make_sph_grid(c["res"], c["ra"], c["dec"], c["radius"])
    assert sorted(g) == ["decpix", "ipix", "npix", "nside", "rapix", "res"] and g["res"] == c["res"] and g["nside"] == 1 << c["res"]
    assert g["ipix"].dtype == np.int64 and g["npix"] == c["npix"] == len(g["ipix"]) == len(g["rapix"]) == len(g["decpix"])
    assert np.array_equal(g["ipix"], G[name + "_ipix"]) and np.all(np.diff(g["ipix"]) > 0)
    disc = H.query_disc(1 << c["res"], R.ang2vec(np.pi / 2.0 - c["dec"], c["ra"]), c["radius"])
    assert disc.dtype == np.int64 and np.array_equal(disc, G[name + "_disc"]) and len(disc) == c["ndisc"]
    # the centres of the hits within the bound of the exact ones
    every = np.union1d(G[name + "_ipix"], G[name + "_disc"])
    at = np.searchsorted(every, g["ipix"])
    bt, bp = angle_bound(G[name + "_err"])
    et, ep = g["decpix"] - (np.pi / 2.0 - G[name + "_theta"][at]), g["rapix"] - G[name + "_phi"][at]
    report(f"{name} dec", np.abs(et), float(bt)), report(f"{name} ra", np.abs(ep), float(bp))
    assert np.all(np.abs(et) <= bt) and np.all(np.abs(ep) <= bp)
    if name == "r5_pole":
        assert g["npix"] == 42 and len(disc) == 44 and set(g["ipix"]) < set(disc)
    if name == "r5_empty":
        assert g["npix"] == 0 and g["ipix"].shape == (0,) and g["rapix"].shape == (0,) and disc.shape == (0,)


def test_seeded_caps_equal_brute_force_over_every_pixel():
    from pyimcom_amd import healpix as H

    theta, phi = R.pix2ang(64, np.arange(49152))
    counts = []
    for ra, dec, radius in seeded_caps():
        brute = np.nonzero(R.cap_mu(ra, dec, theta, phi) >= np.cos(radius))[0]
        got = H.query_disc(64, R.ang2vec(np.pi / 2.0 - dec, ra), radius)
        assert np.array_equal(got, brute), (ra, dec, radius, len(got), len(brute))
        counts.append(len(got))
    assert min(counts) >= 1 and max(counts) > 4000


def test_generate_star_grid_against_the_fixture():
    from pyimcom_amd import healpix as H

    w = grid_wcs()
    ipix, px, py, ra, dec = H.generate_star_grid(META["grid"]["res"], w)
    assert all(isinstance(a, np.ndarray) for a in (ipix, px, py, ra, dec)) and ipix.dtype == np.int64
    assert np.array_equal(ipix, G["grid_ipix"]) and len(ipix) == META["grid"]["npix"]
    x2, y2 = w.all_world2pix(ra, dec, 0)
    assert np.array_equal(px, x2) and np.array_equal(py, y2)
    ex, ey = np.abs(px - G["grid_xy"][:, 0]), np.abs(py - G["grid_xy"][:, 1])
    bound = 10 * G["grid_err"]
    report("star grid x", ex, bound[0]), report("star grid y", ey, bound[1])
    assert np.all(ex <= bound[0]) and np.all(ey <= bound[1])
    # the degrees are the radians over pi / 180, one division; a header mapping is taken like a DeviceWCS
    g = H.make_sph_grid(META["grid"]["res"], *META["grid"]["centre"], 4088 * 0.11 / 3600 * (np.pi / 180))
    assert np.array_equal(g["ipix"], ipix) and np.array_equal(ra, g["rapix"] / (np.pi / 180)) and np.array_equal(dec, g["decpix"] / (np.pi / 180))
    again = H.generate_star_grid(META["grid"]["res"], META["grid"]["header"])
    assert all(np.array_equal(a, b) for a, b in zip(again, (ipix, px, py, ra, dec)))


def test_block_star_grid_against_the_fixture():
    from pyimcom_amd import healpix as H

    b, w = META["block"], block_wcs()
    g = H.block_star_grid(b["res"], w, b["n"], b["bdpad"], b["search_radius"], position_angle=True)
    assert sorted(g) == ["dec", "ipix", "pa", "ra", "x", "xi", "y", "yi"]
    assert np.array_equal(g["ipix"], G["block_ipix"]) and len(g["ipix"]) == b["npix"]
    kept = np.isin(G["block_disc"], G["block_ipix"])  # (the fixture's xi, yi are those of the whole disc, analysis.py:967-968)
    assert g["xi"].dtype == np.int16 and np.array_equal(g["xi"], G["block_xi"][kept]) and np.array_equal(g["yi"], G["block_yi"][kept])
    assert np.all((g["xi"] >= b["bdpad"]) & (g["xi"] < b["n"] - b["bdpad"]) & (g["yi"] >= b["bdpad"]) & (g["yi"] < b["n"] - b["bdpad"]))
    x2, y2 = w.all_world2pix(g["ra"], g["dec"], 0)
    assert np.array_equal(g["x"], x2) and np.array_equal(g["y"], y2)
    lon, lat = H.pix2ang(1 << b["res"], g["ipix"], lonlat=True)
    assert np.array_equal(g["ra"], lon) and np.array_equal(g["dec"], lat)
    bound = 10 * G["block_err"]
    ex, ey = np.abs(g["x"] - G["block_xy"][:, 0]), np.abs(g["y"] - G["block_xy"][:, 1])
    epa = np.abs(g["pa"] - G["block_pa_exact"])
    epa = np.minimum(epa, 360.0 - epa)
    report("block x", ex, bound[0]), report("block y", ey, bound[1]), report("block pa", epa, bound[2])
    assert np.all(ex <= bound[0]) and np.all(ey <= bound[1]) and np.all(epa <= bound[2])
    assert np.all((g["pa"] >= 0) & (g["pa"] < 360))
    # without the box the selection is the disc; without the angle there is no "pa"
    disc = H.query_disc(1 << b["res"], H.ang2vec(*w.all_pix2world([[(b["n"] - 1) / 2] * 2], 0)[0], lonlat=True), b["search_radius"])
    assert np.array_equal(disc, G["block_disc"]) and len(disc) == b["ndisc"]
    assert "pa" not in H.block_star_grid(b["res"], b["header"], b["n"], b["bdpad"], b["search_radius"])


def test_two_runs_give_the_same_bits_and_device_results_stay_on_the_device(monkeypatch):
    import torch

    from pyimcom_amd import healpix as H

    def same_bits(a, b):
        return a.dtype == b.dtype and torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)

    b, w = META["block"], block_wcs()
    first, second = (H.block_star_grid(b["res"], w, b["n"], b["bdpad"], b["search_radius"], position_angle=True, device_out=True) for _ in range(2))
    grid = H.generate_star_grid(META["grid"]["res"], grid_wcs(), device_out=True)
    c = CAPS["r14_wrap"]
    cap1 = H.make_sph_grid(c["res"], c["ra"], c["dec"], c["radius"], device_out=True)

    # where the centre is given, nothing comes to the host: Tensor.cpu, Tensor.numpy and Tensor.tolist are taken away
    def refuse(*a, **k):
        raise AssertionError("a device result was brought to the host")

    for name in ("cpu", "numpy", "tolist"):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    cap2 = H.make_sph_grid(c["res"], c["ra"], c["dec"], c["radius"], device_out=True)
    p = cap2["ipix"]
    theta, phi = H.pix2ang(1 << c["res"], p)  # a tensor in, tensors out
    back = H.ang2pix(1 << c["res"], theta, phi)
    disc = H.query_disc(64, [0.0, 0.6, 0.8], 0.2, device_out=True)
    monkeypatch.undo()
    for t in list(second.values()) + [cap2["ipix"], cap2["rapix"], cap2["decpix"], theta, phi, back, disc] + list(grid):
        assert isinstance(t, torch.Tensor) and t.is_cuda
    assert torch.equal(back, p) and same_bits(phi, cap2["rapix"])
    assert sorted(first) == sorted(second) and all(same_bits(first[k], second[k]) for k in first)
    assert all(same_bits(cap1[k], cap2[k]) for k in ("ipix", "rapix", "decpix"))
    assert np.array_equal(grid[0].cpu().numpy(), G["grid_ipix"]) and np.array_equal(cap2["ipix"].cpu().numpy(), G["r14_wrap_ipix"])


def test_inject_takes_the_device_grid(golden):
    from pyimcom_amd import healpix as H
    from pyimcom_amd import inject

    g = golden("inject")
    oversamp, psf = int(g["oversamp"]), np.ascontiguousarray(g["anlsim_psfs"][0])
    w, res, nside = grid_wcs(), 11, 4088
    ipix, px, py, ra, dec = H.generate_star_grid(res, w)
    on = np.nonzero(inject.on_chip(px, py, nside))[0]
    assert 3 <= on.size < ipix.size  # some of the cap's points reach the chip, some do not
    seen = []

    def inpsf(pos, use_drawpsf=False):
        seen.append(pos)
        return psf

    got = inject.make_image_from_grid(res, inpsf, (0, 1), None, w, nside, oversamp, star_grid=H.generate_star_grid)
    want = inject.star_image(px, py, nside, oversamp, psf_fn=lambda i: psf).cpu().numpy()
    assert got.shape == (nside, nside) and np.array_equal(got, want) and np.count_nonzero(got) > 0
    assert {(float(a), float(b)) for a, b in seen} == {(float(ra[i]), float(dec[i])) for i in on}


def test_entries_take_host_arrays_too():
    """The C entries with IMCOM_MEM_HOST: numpy arrays in and out through the context's workspace, the bits of the device-array calls."""
    import ctypes as C

    from pyimcom_amd import healpix as H
    from pyimcom_amd._lib import MEM_HOST, check, default_context, lib, ptr

    ctx = default_context(0)
    p = np.ascontiguousarray(G["res29_ipix"])
    a, b = np.empty(p.size), np.empty(p.size)
    check(lib.imcom_healpix_pix2ang(ctx.handle, 29, ptr(p), p.size, 0, ptr(a), ptr(b), MEM_HOST))
    theta, phi = H.pix2ang(1 << 29, p)
    assert np.array_equal(a, theta) and np.array_equal(b, phi)
    back = np.empty(p.size, dtype=np.int64)
    check(lib.imcom_healpix_ang2pix(ctx.handle, 29, ptr(a), ptr(b), p.size, 0, ptr(back), MEM_HOST))
    assert np.array_equal(back, p)
    blk, w = META["block"], block_wcs()
    want = H.block_star_grid(blk["res"], w, blk["n"], blk["bdpad"], blk["search_radius"], position_angle=True)
    ra, dec = blk["centre"]
    count = C.c_long(0)
    args = (ctx.handle, blk["res"], ra, dec, blk["search_radius"], 1, 1, ptr(w.descriptor), None, 0, 0, 0.0, 0.0, 0, blk["n"], blk["bdpad"])
    check(lib.imcom_healpix_cap(*args, 0, None, None, None, None, None, None, None, None, C.byref(count), MEM_HOST))
    n = count.value
    assert n == blk["npix"]
    ipix = np.empty(n, dtype=np.int64)
    out = [np.empty(n) for _ in range(7)]  # ra, dec (radians), ra, dec (degrees), x, y, pa
    check(lib.imcom_healpix_cap(*args, n, ptr(ipix), *[ptr(o) for o in out], C.byref(count), MEM_HOST))
    assert np.array_equal(ipix, want["ipix"])
    for got, key in zip(out[2:], ("ra", "dec", "x", "y", "pa")):
        assert np.array_equal(got, want[key]), key
    assert np.array_equal(out[0], H.pix2ang(1 << blk["res"], ipix)[1])
    # room that is not the count is refused before anything is written
    assert lib.imcom_healpix_cap(*args, n - 1, ptr(ipix), None, None, None, None, None, None, None, None, MEM_HOST) == -1
