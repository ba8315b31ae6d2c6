"""The star catalog on the device (pyimcom_amd.starcat, csrc/starmom.hip) against tests/golden/starcat.npz -- the reference's own statements
with the float64 restatement of the adaptive moments standing in for GalSim -- and against the restatement itself (tests/starcat_reference.py).

Tolerances are derived, not tuned.  A float64 sum of n = 6241 terms in any order is within n 2^-53, about 7e-13, of the sum of the terms'
magnitudes; the iteration contracts by about one half a step, so it does not amplify that by more than about 2: 1e-11 times the column's
scale stored with the golden (the flux for the amplitude, sigma for centroid and width, 1 for the shapes, sum |terms| / |sum of weights| for
the four ratio columns), with equal iteration counts required.  The window means of integer-coded maps are exact; those of float maps are
within 1e-14 relative of numpy's on the window cast to float64 and within 225 x 2^-24 of the reference's float32 accumulation."""

import os

import numpy as np
import pytest

from tests import starcat_reference as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(ROOT, "tests", "golden", "starcat.npz"))
BDS = [int(b) for b in G["bds"]]
TOL = 1e-11
NAMES = R.COLUMNS[4:14]


@pytest.fixture(scope="module")
def SC():
    import __graft_entry__ as g

    g.build()
    from pyimcom_amd import starcat

    return starcat


def _kw():
    return dict(forced_scale=float(G["forced_scale"]), fidelity=(G["fid"], float(G["bels"])), inweight=G["inweight"], n2=int(G["n2"]), uc=G["uc"], sigma=G["sigma"],
                tsum=G["tsum"], neff=G["neff"])


def _check_moments(m, bd, who):
    mom, rows, scale = G[f"mom_{bd}"], G[f"rows_{bd}"], G[f"scale_{bd}"]
    status, n_iter = np.asarray(m["status"]), np.asarray(m["n_iter"])
    print(who, bd, "status", status, "iterations", n_iter)
    assert np.array_equal(status, mom[:, 10].astype(np.int32)), (who, status, mom[:, 10])
    ok = status == 0
    assert np.array_equal(n_iter[ok], mom[ok, 9].astype(np.int32)), (who, n_iter, mom[:, 9])
    for j, name in enumerate(NAMES):
        got, want = np.asarray(m[name]), rows[:, 10 + j]
        err = np.abs(got[ok] - want[ok]) / scale[ok, j]
        print(who, bd, name, "largest error in units of the scale", err.max() if err.size else 0.0)
        assert np.all(err <= TOL), (who, name, err)
        assert np.all(got[~ok] == 0.0), (who, name)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("bd", BDS)
def test_golden_moments_numpy_and_tensor(SC, bd, dtype):
    import torch

    frame = G["frame"].astype(dtype)
    m = SC.star_moments(frame, G["x"], G["y"], bd, float(G["forced_scale"]))
    assert isinstance(m["AMPLITUDE"], np.ndarray)
    _check_moments(m, bd, f"numpy {np.dtype(dtype).name}")
    wide = torch.zeros((96, 131), dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda:0")
    wide[:, 3:99] = torch.as_tensor(frame).to("cuda:0")
    mt = SC.star_moments(wide[:, 3:99], G["x"], G["y"], bd, float(G["forced_scale"]))  # (a view with a pitch: read in place)
    assert mt["AMPLITUDE"].is_cuda and mt["table"].shape == (len(G["x"]), SC.NCOL)
    assert np.array_equal(mt["table"].cpu().numpy(), m["table"], equal_nan=True)
    _check_moments({k: v.cpu().numpy() for k, v in mt.items()}, bd, "tensor")


@pytest.mark.parametrize("bd", BDS)
def test_golden_catalog_and_starcube_rows(SC, bd):
    fits = G[f"fits_{bd}"]
    scale = G[f"scale_{bd}"]
    cat = SC.star_catalog(G["frame"], G["x"][fits], G["y"][fits], bd=bd, bd2=int(G["bd2"]), ra=G["ra"][fits], dec=G["dec"][fits], **_kw())
    want = G[f"cat_{bd}"]
    assert cat.shape == want.shape == (len(fits), 20) and np.array_equal(cat[:, :4], want[:, :4])
    ok = G[f"mom_{bd}"][fits, 10] == 0
    assert np.all(np.abs(cat[:, 4:14] - want[:, 4:14])[ok] <= TOL * scale[fits][ok]) and np.all(cat[~ok, 4:] == 0) and np.all(want[~ok, 4:] == 0)
    assert np.array_equal(cat[:, 14:16], want[:, 14:16])  # FIDELITY (integers summed), COVERAGE: exact
    for j in (16, 17, 18, 19):  # the reference accumulates these float32 windows in float32
        assert np.all(np.abs(cat[ok, j] - want[ok, j]) <= 225 * 2.0 ** -24 * np.abs(want[ok, j])), (j, cat[:, j], want[:, j])
    import torch

    dev = {k: (torch.as_tensor(v.view(np.int16) if v.dtype == np.uint16 else v).to("cuda:0") if isinstance(v, np.ndarray) else v) for k, v in _kw().items()}
    dev["fidelity"] = (torch.as_tensor(G["fid"].view(np.int16)).to("cuda:0"), float(G["bels"]))
    tcat = SC.star_catalog(torch.as_tensor(G["frame"]).to("cuda:0"), G["x"][fits], G["y"][fits], bd=bd, bd2=int(G["bd2"]), ra=G["ra"][fits], dec=G["dec"][fits], **dev)
    assert tcat.is_cuda and np.array_equal(tcat.cpu().numpy(), cat, equal_nan=True)  # frames and maps on the device: the table stays there, the same bits
    emp = SC.star_catalog(G["frame"], G["x"][fits], G["y"][fits], bd=bd, bd2=int(G["bd2"]), ra=G["ra"][fits], dec=G["dec"][fits], empirical=True,
                          **{**_kw(), "sigma": None, "neff": None})
    wemp = G[f"cat_empirical_{bd}"]
    assert np.array_equal(emp[:, [17, 18, 19]], wemp[:, [17, 18, 19]]) and np.array_equal(emp[:, 4:14], cat[:, 4:14])  # -1, 0, -1 (zeros for a failed star)
    kw = _kw()
    pos, cube = SC.starcube_rows(G["frame"], G["x"], G["y"], 3, 5, bd=bd, bd2=int(G["bd2"]), force_scale=kw["forced_scale"], fidelity=kw["fidelity"],
                                 inweight=kw["inweight"], n2=kw["n2"], ra=G["ra"], dec=G["dec"])
    rows = G[f"rows_{bd}"]
    allok = G[f"mom_{bd}"][:, 10] == 0
    assert pos.shape == rows.shape and np.array_equal(pos[:, :10], rows[:, :10]) and np.array_equal(pos[:, 20:], rows[:, 20:], equal_nan=True)  # (NaN: the window of the star at the frame's edge is an empty slice)
    assert np.all(np.abs(pos[:, 10:20] - rows[:, 10:20])[allok] <= TOL * G[f"scale_{bd}"][allok]) and np.all(pos[~allok, 10:] == 0)
    assert cube.dtype == np.float32 and np.array_equal(cube, G[f"cube_{bd}"])


def _images():
    return {"7x7": R.draw_star(7, 3.2, 2.9, 1.5, 1.1, 0.1, 0.05, 0.0), "10x12": R.draw_star(12, 5.7, 4.4, 2.0, 1.4, -0.1, 0.1, 0.0)[:10],
            "79x79": R.draw_star(79, 39.3, 38.6, 1.7, 3.1, 0.25, -0.1, 0.0)}


@pytest.mark.parametrize("which", ["7x7", "10x12", "79x79"])
def test_adaptive_moments_of_images_with_odd_and_even_sides(SC, which):
    import torch

    img = _images()[which]
    want = R.find_adaptive_mom(img)
    assert want.error_message == ""
    both = np.stack([img, img[::-1, ::-1]])
    got = SC.adaptive_moments(both)
    one = SC.adaptive_moments(torch.as_tensor(img).to("cuda:0"))
    assert one.single and one.moments_amp.is_cuda and np.array_equal(one.table.cpu().numpy()[0], got.table[0])
    flux, sig = abs(want.moments_amp), want.moments_sigma
    print(which, "iterations", got.moments_n_iter, want.moments_n_iter, "amp", got.moments_amp[0] - want.moments_amp, "sigma", got.moments_sigma[0] - want.moments_sigma)
    assert got.error_message == ["", ""] and got.moments_n_iter[0] == want.moments_n_iter
    assert abs(got.moments_amp[0] - want.moments_amp) <= TOL * flux and abs(got.moments_sigma[0] - want.moments_sigma) <= TOL * sig
    assert abs(got.moments_centroid_x[0] - want.moments_centroid.x) <= TOL * sig and abs(got.moments_centroid_y[0] - want.moments_centroid.y) <= TOL * sig
    for name in ("e1", "e2", "g1", "g2"):
        assert abs(getattr(got, name)[0] - getattr(want.observed_shape, name)) <= TOL
    assert abs(got.moments_rho4[0] - want.moments_rho4) <= 625 * TOL  # (rho2^2 <= 25^2 under the sum)
    h, w = img.shape  # the image turned by half a turn: the centroid mirrored, e unchanged
    assert abs(got.moments_centroid_x[1] - (w + 1 - want.moments_centroid.x)) <= 1e-9 * sig and abs(got.e1[1] - want.observed_shape.e1) <= 1e-9


def test_failures_give_their_status_and_the_call_returns(SC):
    zero = np.zeros((3, 15, 15), dtype=np.float32)
    zero[1] = R.cut(G["frame"], 42, 14, 8)
    zero[2, 0, 0] = np.nan
    got = SC.adaptive_moments(zero)
    assert list(got.moments_status) == [R.STATUS_NAN, 0, R.STATUS_NAN] and got.error_message[0] == R.MESSAGES[R.STATUS_NAN] and got.error_message[1] == ""
    assert got.moments_sigma[0] == -1 and got.moments_amp[0] == 0 and got.moments_n_iter[0] == 1
    few = SC.adaptive_moments(zero[1], SC.AdaptiveMomParams(max_mom2_iter=3))
    assert few.moments_status[0] == R.STATUS_TOO_MANY and few.moments_n_iter[0] == 4
    m = SC.star_moments(G["frame"], G["x"][[6, 7]], G["y"][[6, 7]], 40, float(G["forced_scale"]))
    assert list(m["status"]) == [R.STATUS_TOO_LARGE, int(G["mom_40"][7, 10])] and all(np.all(m[n] == 0) for n in NAMES)


def test_a_side_of_129_is_refused(SC):
    from pyimcom_amd._lib import ImcomError

    with pytest.raises(ImcomError) as e:
        SC.star_moments(np.zeros((300, 300), dtype=np.float32), [150.0], [150.0], 65)
    assert e.value.status == -4 and "127" in str(e.value)  # IMCOM_ERR_UNSUPPORTED
    with pytest.raises(ImcomError) as e:
        SC.adaptive_moments(np.zeros((129, 20)))
    assert e.value.status == -4
    assert SC.star_moments(np.zeros((300, 300), dtype=np.float32), [150.0], [150.0], 64)["status"][0] == R.STATUS_NAN  # side 127 is served


def _big():
    """A 512 x 512 frame with 257 stars on a grid of 28 px, each its own shape and sub-pixel position."""
    rng = np.random.default_rng(257)
    gx, gy = np.meshgrid(20 + 28 * np.arange(17), 20 + 28 * np.arange(17))
    x = gx.ravel()[:257] + rng.uniform(-0.49, 0.49, 257)
    y = gy.ravel()[:257] + rng.uniform(-0.49, 0.49, 257)
    frame = np.zeros((512, 512))
    yy, xx = np.mgrid[0:21, 0:21].astype(np.float64)
    for k in range(257):
        cx, cy = int(np.rint(x[k])), int(np.rint(y[k]))
        e1, e2 = rng.uniform(-0.2, 0.2, 2)
        frame[cy - 10:cy + 11, cx - 10:cx + 11] = R.draw_star(21, x[k] - cx + 10, y[k] - cy + 10, rng.uniform(1, 5), rng.uniform(1.5, 2.5), e1, e2, 0.0)
    return frame.astype(np.float32), x, y


@pytest.fixture(scope="module")
def big():
    return _big()


def test_batches_of_0_1_and_257_stars_are_the_same_bits(SC, big):
    frame, x, y = big
    fs = float(G["forced_scale"])
    none = SC.star_moments(frame, x[:0], y[:0], 8, fs)
    assert none["table"].shape == (0, SC.NCOL) and none["status"].shape == (0,)
    assert SC.star_catalog(frame, x[:0], y[:0], bd=8, **_kw()).shape == (0, 20)
    full = SC.star_moments(frame, x, y, 8, fs)
    again = SC.star_moments(frame, x, y, 8, fs)
    assert np.all(full["status"] == 0) and full["table"].shape == (257, SC.NCOL)
    assert np.array_equal(full["table"], again["table"])  # two runs: the same bits
    for k in (0, 100, 256):
        alone = SC.star_moments(frame, x[k:k + 1], y[k:k + 1], 8, fs)
        assert np.array_equal(alone["table"][0], full["table"][k]), k  # alone and inside the 257: the same bits
    xi, yi = np.rint(x).astype(int), np.rint(y).astype(int)
    for k in (0, 1, 16, 17, 100, 255, 256):
        cut = R.cut(frame, xi[k], yi[k], 8)
        want = R.find_adaptive_mom(cut)
        cols, _, hscales = R.higher_moments(cut, want, fs)
        assert full["n_iter"][k] == want.moments_n_iter and abs(full["AMPLITUDE"][k] - want.moments_amp) <= TOL * 5.0
        assert abs(full["WIDTH"][k] - want.moments_sigma) <= TOL * want.moments_sigma
        assert np.all(np.abs(np.array([full[n][k] for n in NAMES[6:]]) - cols) <= TOL * hscales)


def test_window_statistics(SC):
    import torch

    x, y = G["x"], G["y"]
    xi, yi = np.rint(x).astype(np.int16), np.rint(y).astype(np.int16)
    xi2, yi2 = np.concatenate([xi, [95, 3, 50]]), np.concatenate([yi, [95, 50, 200]])  # clipped at the far corner; a negative start and a window off the map: empty
    bd2 = int(G["bd2"])
    win = [np.s_[int(b) + 1 - bd2:int(b) + bd2, int(a) + 1 - bd2:int(a) + bd2] for a, b in zip(xi2, yi2)]
    fmap = R.fidelity_map(G["fid"], float(G["bels"]))
    table = SC.fidelity_table(np.uint16, float(G["bels"]))
    with np.errstate(all="ignore"):
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = np.array([np.mean(fmap[w]) for w in win])
            mean, std = SC.window_stats(G["fid"], xi2, yi2, bd2, table=table)
            fin = ~np.isnan(want)
            assert np.array_equal(mean, want, equal_nan=True) and list(np.nonzero(~fin)[0]) == [8, 11, 12]  # exactly numpy's; star 8 at the edge: an empty slice too
            wstd = np.array([np.std(fmap[w].astype(np.float64)) for w in win])
            assert np.allclose(std[fin], wstd[fin], rtol=1e-14, atol=0) and np.isnan(std[~fin]).all()
            for key in ("uc", "sigma", "tsum", "neff"):
                for dtype in (np.float32, np.float64):
                    mp = G[key].astype(dtype)
                    src = torch.as_tensor(mp).to("cuda:0") if dtype == np.float64 else mp
                    mean, std = SC.window_stats(src, xi2, yi2, bd2)
                    mean, std = (mean.cpu().numpy(), std.cpu().numpy()) if dtype == np.float64 else (mean, std)
                    m64 = np.array([np.mean(mp[w].astype(np.float64)) for w in win])
                    s64 = np.array([np.std(mp[w].astype(np.float64)) for w in win])
                    e_m, e_s = np.abs(mean - m64)[fin] / np.abs(m64[fin]), np.abs(std - s64)[fin] / np.abs(s64[fin])
                    print(key, np.dtype(dtype).name, "mean", e_m.max(), "std", e_s.max())
                    assert np.all(e_m <= 1e-14) and np.all(e_s <= 1e-14) and np.isnan(mean[~fin]).all()
                    m32 = np.array([np.mean(G[key][w]) for w in win])  # the reference's own accumulation, in float32
                    s32 = np.array([np.std(G[key][w]) for w in win])
                    assert np.all(np.abs(mean - m32)[fin] <= 225 * 2.0 ** -24 * np.abs(m32[fin])) and np.all(np.abs(std - s32)[fin] <= 225 * 2.0 ** -24 * np.abs(m32[fin]))
    hist = SC.fidelity_histogram(G["fid"], float(G["bels"]), int(G["bdpad"]))
    assert hist.shape == (81,) and np.array_equal(hist, G["fhist"])
    hist_t = SC.fidelity_histogram(torch.as_tensor(G["fid"].view(np.int16)).to("cuda:0"), float(G["bels"]), int(G["bdpad"]))
    assert np.array_equal(hist_t, G["fhist"])


def test_exported_cuts_are_the_padded_slices(SC, big):
    import torch

    xi, yi = np.rint(G["x"]).astype(int), np.rint(G["y"]).astype(int)
    xi, yi = np.concatenate([xi, [-30, 200]]), np.concatenate([yi, [50, -7]])  # off the frame: partly, and altogether
    for bd in BDS:
        want = np.stack([np.pad(G["frame"], 300)[300 + b + 1 - bd:300 + b + bd, 300 + a + 1 - bd:300 + a + bd] for a, b in zip(xi, yi)])
        got = SC.star_cuts(G["frame"], xi, yi, bd)
        assert got.dtype == np.float32 and np.array_equal(got, want) and np.array_equal(got[:10], G[f"cube_{bd}"])
        got64 = SC.star_cuts(torch.as_tensor(G["frame"].astype(np.float64)).to("cuda:0"), xi, yi, bd)
        assert got64.is_cuda and got64.dtype == torch.float32 and np.array_equal(got64.cpu().numpy(), want)
    frame, x, y = big
    k = np.rint(x).astype(int), np.rint(y).astype(int)
    assert np.array_equal(SC.star_cuts(frame, k[0], k[1], 8), np.stack([R.cut(frame, a, b, 8) for a, b in zip(*k)]))


def test_host_arrays_through_the_c_entries_give_the_same_bits(SC):
    """memspace = host: the library stages the caller's numpy arrays itself; the numbers are those of the device path."""
    import ctypes as C

    from pyimcom_amd import _lib

    ctx = _lib.default_context(0)
    frame, bd, bd2 = np.ascontiguousarray(G["frame"]), 8, int(G["bd2"])
    xi, yi = np.rint(G["x"]).astype(np.int32), np.rint(G["y"]).astype(np.int32)
    ox, oy, n, side = xi + 1 - bd, yi + 1 - bd, len(xi), 2 * bd - 1
    sz = (C.c_long * 4)()
    _lib.check(_lib.lib.imcom_star_sizes(n, side, side, 0, sz))
    assert list(sz)[1:3] == [SC.MAX_SIDE, SC.NCOL] and sz[0] >= n * (8 + 8 * SC.NCOL) and sz[3] >= side * side * 4
    out = np.zeros((n, SC.NCOL))
    _lib.check(_lib.lib.imcom_star_moments(ctx.handle, _lib.ptr(frame), 0, 96, 96, 96, _lib.ptr(ox), _lib.ptr(oy), n, side, side, None, float(G["forced_scale"]),
                                           _lib.ptr(out), _lib.MEM_HOST))  # (no parameters: the defaults)
    assert np.array_equal(out, SC.star_moments(frame, G["x"], G["y"], bd, float(G["forced_scale"]))["table"], equal_nan=True)
    cuts = np.zeros((n, side, side), dtype=np.float32)
    _lib.check(_lib.lib.imcom_star_cuts(ctx.handle, _lib.ptr(frame), 0, 96, 96, 96, _lib.ptr(ox), _lib.ptr(oy), n, side, side, _lib.ptr(cuts), _lib.MEM_HOST))
    assert np.array_equal(cuts, G[f"cube_{bd}"])
    table = np.ascontiguousarray(SC.fidelity_table(np.uint16, float(G["bels"])))
    for kind, mp, tab in ((2, np.ascontiguousarray(G["fid"]), table), (0, np.ascontiguousarray(G["tsum"]), None), (1, G["tsum"].astype(np.float64), None)):
        st = np.zeros((n, 2))
        _lib.check(_lib.lib.imcom_star_window_stats(ctx.handle, _lib.ptr(mp), kind, 96, 96, 96, _lib.ptr(tab), _lib.ptr(xi), _lib.ptr(yi), n, bd2, _lib.ptr(st), _lib.MEM_HOST))
        mean, std = SC.window_stats(mp, xi, yi, bd2, table=tab)
        assert np.array_equal(st[:, 0], mean, equal_nan=True) and np.array_equal(st[:, 1], std, equal_nan=True)
