"""pyimcom_amd.objmask on the device (csrc/objmask.hip) against numpy, against the reference's own outputs (tests/golden/objmask.npz, made
with scipy) and, beyond the fixture, against the numpy restatement that tests/test_objmask_host.py pins to it.  Every comparison is exact
equality: the results are booleans, counts and order statistics, and the scalar steps between the kernels are numpy's own on the host."""

import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import objmask_reference as R
from tests.test_destripe_host import GOLDEN, load_case
from tests.test_objmask_host import CASES, G, MASKS, SCALARS, edge_inputs, same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (1, 2, 3, 255, 256, 257, 65537)
DTYPES = [np.float32, np.float64]


def _np_median(a):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.median(a)


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


# ---- selection ----
@pytest.mark.parametrize("dtype", DTYPES)
def test_median_equals_numpys(dtype):
    import torch

    from pyimcom_amd import objmask

    inputs = edge_inputs(dtype)
    assert {int(k.split("_")[1]) for k in inputs} == set(SIZES)
    for name, a in inputs.items():
        want = _np_median(a)
        assert same(objmask.median(a), want), name
        if name.startswith("nan_"):
            assert np.isnan(want)
    a = inputs["levels_65537"]
    assert np.unique(a).size == 7 and np.sort(a)[a.size // 2 - 1] == np.sort(a)[a.size // 2 + 1]  # the middle lies inside a run of ties
    assert same(objmask.median(torch.as_tensor(a, device=DEV).reshape(1, -1)), _np_median(a))  # a tensor, any shape
    assert same(objmask.median(a), objmask.median(a))


@pytest.mark.parametrize("dtype", DTYPES)
def test_order_statistics_equal_numpys_partition(dtype):
    from pyimcom_amd import objmask

    for name, a in edge_inputs(dtype).items():
        n = a.size
        for k in sorted({0, (n - 1) // 2, n // 2, n - 1}):
            want = np.partition(a, sorted({k, min(k + 1, n - 1)}))
            lo, hi = objmask.order_statistics(a, k)
            assert same(lo, want[k]) and same(hi, want[min(k + 1, n - 1)]), (name, k)
    with pytest.raises(ValueError):
        objmask.order_statistics(np.zeros(4, dtype=dtype), 4)


@pytest.mark.parametrize("dtype", DTYPES)
def test_median_of_a_flagged_subset_and_of_absolute_differences(dtype):
    from pyimcom_amd import objmask

    rng = np.random.default_rng(4)
    inputs = edge_inputs(dtype)
    for n in (257, 65537):
        for kind in ("levels", "ulps", "zeros", "inf"):
            a = inputs[f"{kind}_{n}"]
            for keep in (1, 2, n // 2):
                f = np.zeros(n, dtype=bool)
                f[rng.choice(n, size=keep, replace=False)] = True
                assert same(objmask.median(a, where=f), _np_median(a[f])), (kind, n, keep)
                assert same(objmask.median(a, where=f.view(np.uint8)), _np_median(a[f]))
            c = _np_median(a[np.isfinite(a)])
            with np.errstate(invalid="ignore"):
                want = _np_median(np.abs(a - c))
            assert same(objmask.median(a, center=c), want), (kind, n)
            f = np.isfinite(a) & (rng.uniform(size=n) < 0.5)
            assert same(objmask.median(a, where=f, center=c), _np_median(np.abs(a[f] - c))), (kind, n)
    assert np.isnan(objmask.median(inputs["levels_257"], where=np.zeros(257, dtype=bool)))  # nothing flagged, as np.median of nothing


def test_selection_entry_with_host_arrays_and_its_refusals():
    from pyimcom_amd import _lib

    ctx = _lib.default_context()
    a = edge_inputs(np.float64)["levels_257"]
    out, info = np.zeros(2), np.zeros(2, dtype=np.int64)

    def call(n, k=-1, vals=a):
        return _lib.lib.imcom_select_kth(ctx.handle, _lib.ptr(vals), 1, n, None, 0, 0.0, k, _lib.ptr(out), _lib.ptr(info), _lib.MEM_HOST)

    assert call(257) == 0
    assert out[0] == out[1] == np.median(a) and list(info) == [257, 0]
    assert call(256) == 0 and np.mean(out) == np.median(a[:256])
    assert call(0) == -1 and "select_kth" in _lib.lib.imcom_last_error().decode()  # IMCOM_ERR_ARG
    assert call(257, k=257) == -1
    assert _lib.lib.imcom_select_kth(None, _lib.ptr(a), 1, 257, None, 0, 0.0, -1, _lib.ptr(out), _lib.ptr(info), _lib.MEM_HOST) == -1
    assert "null context" in _lib.lib.imcom_last_error().decode()


# ---- dilation ----
@pytest.mark.parametrize("name", ["corners", "edges_tiles", "row"])
def test_dilation(name):
    import torch

    from pyimcom_amd import _lib, objmask

    a = G[f"dil_{name}"]
    assert a.shape == (150, 203) and objmask.DILATE_TILE == (32, 48)  # the fixture's pixels at (31, 47), (32, 48), (63, 96), (64, 95) straddle tiles
    got = {}
    for r in (1, 2, 4):
        got[r] = objmask.dilate(a, r)
        assert got[r].dtype == np.bool_ and np.array_equal(got[r], G[f"dil_{name}_r{r}"]), r
        assert np.array_equal(got[r], R.dilate(a, r))
    assert np.array_equal(objmask.dilate(got[2], 2), got[4])
    dev = objmask.dilate(torch.as_tensor(a, device=DEV), 2)
    assert dev.is_cuda and dev.dtype == torch.bool and np.array_equal(dev.cpu().numpy(), got[2])
    with pytest.raises(_lib.ImcomError) as e:
        objmask.dilate(a, 9)
    assert e.value.status == -4  # IMCOM_ERR_UNSUPPORTED
    src, dst = np.ascontiguousarray(a).view(np.uint8), np.zeros(a.shape, dtype=np.uint8)
    ctx = _lib.default_context()
    for r, status in ((9, -4), (0, -4), (8, 0)):
        assert _lib.lib.imcom_mask_dilate(ctx.handle, _lib.ptr(src), 150, 203, r, _lib.ptr(dst), _lib.MEM_HOST) == status
    assert np.array_equal(dst.view(np.bool_), R.dilate(a, 8))


# ---- propagation ----
def _propagation_scene():
    """200 x 203 with tiles of 62: (grow, seed, points that must be reached, points that must stay off)."""
    from pyimcom_amd import objmask

    T = objmask.PROPAGATE_TILE
    H, W = 200, 203
    assert T == 62 and H > 3 * T and W > 3 * T and H % T and W % T
    grow, seed = np.zeros((H, W), dtype=bool), np.zeros((H, W), dtype=bool)
    for k, y in enumerate(range(0, 119, 2)):  # a one-pixel serpentine over two tile rows: every run crosses four tiles
        grow[y, :] = True
        if y + 2 < 119:
            grow[y + 1, W - 1 if k % 2 == 0 else 0] = True
    seed[0, 0] = True
    far = [(118, 0), (118, W - 1), (118, W // 2)]  # the last run, its far end first
    grow[3 * T, 10:191] = True  # along the first row of the last tile row ...
    grow[130:3 * T + 1, 2 * T - 1] = True  # ... joined to the last column of the second tile column
    seed[130, 2 * T - 1] = True
    far += [(3 * T, 10), (3 * T, 190)]
    grow[140:161, 20] = grow[140:161, 40] = grow[140, 20:41] = grow[160, 20:41] = True  # a closed ring, no seed
    off = [(140, 20), (160, 40), (150, 20)]
    grow[140:145, 60:65] = grow[145:150, 65:70] = True  # two blobs that touch by a corner
    seed[142, 62] = True
    far.append((144, 64))
    off += [(145, 65), (149, 69)]
    seed[170, 60] = True  # a seed outside grow ...
    grow[170, 61:64] = True  # ... spreads into its grow neighbours
    far += [(170, 60), (170, 63)]
    off.append((170, 59))
    return grow, seed, far, off


def test_propagation():
    import torch

    from pyimcom_amd import objmask

    grow, seed, far, off = _propagation_scene()
    want = R.propagate(seed, grow)
    got, sweeps = objmask.propagate(seed, grow, return_sweeps=True)
    assert got.dtype == np.bool_ and np.array_equal(got, want)
    assert all(got[p] for p in far) and not any(got[p] for p in off)
    assert sweeps >= 60 * 2  # a run of 203 pixels is longer than two 64-pixel windows, and a sweep moves the front by one window at most
    assert not got[~(grow | seed)].any() and got[seed].all()
    dev = objmask.propagate(torch.as_tensor(seed, device=DEV), torch.as_tensor(grow, device=DEV))
    assert dev.is_cuda and dev.dtype == torch.bool and np.array_equal(dev.cpu().numpy(), want)
    empty, n = objmask.propagate(np.zeros_like(seed), grow, return_sweeps=True)
    assert not empty.any() and n == 2
    assert np.array_equal(objmask.propagate(seed, np.zeros_like(grow)), seed)  # nothing to grow into
    assert np.array_equal(objmask.propagate(G["prop_seed"], G["prop_grow"]), G["prop_out"])  # scipy's own answer
    one = objmask.propagate(np.ones((1, 1), dtype=bool), np.ones((1, 1), dtype=bool))
    assert one.shape == (1, 1) and one.all()


def test_outputs_are_ordered_on_a_side_stream():
    """The seams launch on torch's current stream of the context's device: on a side stream, with no synchronise, a torch op of that
    stream reads what the kernel wrote.  3 x 70 is wider than a 64-bit flood word and crosses a dilation tile's column boundary (48)."""
    import torch

    from pyimcom_amd import objmask, simmask

    mask = np.zeros((3, 70), dtype=bool)
    mask[1, 0] = mask[0, 47] = mask[2, 63] = mask[1, 69] = True
    grow, seed = np.zeros((3, 70), dtype=bool), np.zeros((3, 70), dtype=bool)
    grow[1, :] = seed[1, 0] = grow[0, 69] = grow[2, 30] = True
    side = torch.cuda.Stream(DEV)
    assert side != torch.cuda.default_stream(DEV)
    with torch.cuda.stream(side):
        u = (simmask.uniform(7, 0, (5,), device=DEV) + 0.0).cpu().numpy()
        d = objmask.dilate(torch.as_tensor(mask, device=DEV), 1).logical_or(torch.zeros((), dtype=torch.bool, device=DEV)).cpu().numpy()
        p = objmask.propagate(torch.as_tensor(seed, device=DEV), torch.as_tensor(grow, device=DEV)).clone().cpu().numpy()
    assert u.dtype == np.float64 and np.array_equal(u, np.random.Generator(np.random.PCG64(7)).uniform(size=5))
    assert d.dtype == np.bool_ and np.array_equal(d, R.dilate(mask, 1))
    assert p.dtype == np.bool_ and np.array_equal(p, R.propagate(seed, grow)) and p[1].all() and p[0, 69] and p[2, 30]


# ---- the whole function ----
def _check_details(name, d):
    seen = 0
    for q in SCALARS + MASKS:
        if f"{name}__{q}" in G.files:
            got = _host(d[q])
            got = got.view(np.bool_) if q in MASKS else got
            assert same(got, G[f"{name}__{q}"]), (name, q, got, G[f"{name}__{q}"])
            seen += 1
    return seen


@pytest.mark.parametrize("name", CASES)
def test_apply_object_mask_equals_the_reference(name):
    import torch

    from pyimcom_amd import objmask

    image, (m, c), kind = G[f"{name}__image"], G[f"{name}__pars"], str(G[f"{name}__type"])
    m = int(m) if m == int(m) else float(m)
    d = {}
    out, mask = objmask.apply_object_mask(image.copy(), threshold_m=m, threshold_c=float(c), type=kind, details=d)
    assert isinstance(out, np.ndarray) and mask.dtype == np.bool_ and np.array_equal(mask, G[f"{name}__neighbor_mask"])
    assert same(out, G[f"{name}__image_out"])
    assert _check_details(name, d) >= (2 if kind != "jwst" else 3)
    if name == "jwst_const":
        assert d["std_fallback"] and d["seed_threshold"] == 0.3 and d["grow_threshold"] == 0.15  # max(c, 0), max(c / 2, 0)
    if name == "jwst_small":
        assert d["rounds"] == 0 and d["n_clip"] == 64  # fewer than 100 kept: the first clip is not taken
    if name == "jwst_nonfinite":
        assert d["n_valid"] == 0
    inpl = image.copy()
    out2, mask2 = objmask.apply_object_mask(inpl, threshold_m=m, threshold_c=float(c), inplace=True, type=kind)
    assert out2 is inpl and same(inpl, G[f"{name}__image_out"]) and np.array_equal(mask2, mask)
    # a device tensor in: device tensors out, the same bits
    t = torch.as_tensor(image, device=DEV)
    dout, dmask = objmask.apply_object_mask(t, threshold_m=m, threshold_c=float(c), type=kind)
    assert dout.is_cuda and dmask.is_cuda and dmask.dtype == torch.bool and dout.dtype == t.dtype and dout.data_ptr() != t.data_ptr()
    assert dout.cpu().numpy().tobytes() == out.tobytes() and np.array_equal(dmask.cpu().numpy(), mask)
    assert same(t.cpu().numpy(), image)  # untouched
    dout2, dmask2 = objmask.apply_object_mask(t, threshold_m=m, threshold_c=float(c), inplace=True, type=kind)
    assert dout2 is t and t.cpu().numpy().tobytes() == out.tobytes() and np.array_equal(dmask2.cpu().numpy(), mask)
    given, same_mask = objmask.apply_object_mask(torch.as_tensor(image, device=DEV), mask=dmask, type=kind)  # a given mask is applied as it is
    assert given.cpu().numpy().tobytes() == out.tobytes() and np.array_equal(same_mask.cpu().numpy(), mask)
    given, same_mask = objmask.apply_object_mask(image.copy(), mask=mask, type=kind)
    assert same_mask is mask and same(given, out)


@functools.lru_cache(maxsize=None)
def _large(dtype_name):
    """320 x 320: sky, sources and non-finite pixels, with the restatement's answer (made once)."""
    img = R.scene((320, 320), np.dtype(dtype_name).type, 21 if dtype_name == "float64" else 22, nsrc=14, nonfinite=12)
    d = {}
    out, mask = R.apply_object_mask(img.copy(), threshold_c=0.3, type="jwst", details=d)
    return img, out, mask, d


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_jwst_route_beyond_the_fixture(dtype_name):
    from pyimcom_amd import objmask

    img, want_out, want_mask, want = _large(dtype_name)
    assert np.isinf(img).any() and np.isnan(img).any() and 0 < np.count_nonzero(want_mask) < img.size // 2 and want["n_clip"] < np.isfinite(img).sum()
    d = {}
    out, mask = objmask.apply_object_mask(img.copy(), threshold_c=0.3, type="jwst", details=d)
    assert np.array_equal(mask, want_mask) and same(out, want_out)
    for q in ("bkg", "mad", "sigma", "seed_threshold", "grow_threshold", "n_clip"):
        assert same(d[q], want[q]), q
    for q in ("seed_mask", "grow_candidates", "grown_mask", "high_value_mask"):
        assert np.array_equal(_host(d[q]).view(np.bool_), want[q]), q
    assert d["rounds"] >= 1 and d["sweeps"] >= 2


def test_fits_route_thresholds_and_types():
    from pyimcom_amd import objmask

    for m in (0, 15):
        img = R.fits_scene(threshold_m=m)
        thr = np.float32(R.fits_threshold(img, m, 0.3))
        d = {}
        out, mask = objmask.apply_object_mask(img, threshold_m=m, threshold_c=0.3, details=d)
        want_out, want_mask = R.apply_object_mask(img, threshold_m=m, threshold_c=0.3)
        assert np.array_equal(mask, want_mask) and same(out, want_out) and same(d["threshold"], thr)
        high = _host(d["high_value_mask"]).view(np.bool_)
        assert high[img == thr].all() and (img == thr).sum() == 1  # the pixel on the threshold is in: >=
        assert not high[img == np.nextafter(thr, np.float32(0))].any()
    d = {}
    wide = objmask.apply_object_mask(img, threshold_m=0, threshold_c=np.float64(thr) + 1e-9, details=d)[1]  # a float64 scalar: numpy compares in float64
    assert np.array_equal(wide, R.apply_object_mask(img, threshold_m=0, threshold_c=np.float64(thr) + 1e-9)[1])
    assert not _host(d["high_value_mask"]).view(np.bool_)[img == thr].any()  # rounded to float32 the threshold would let it in
    with pytest.raises(TypeError):
        objmask.apply_object_mask(np.zeros((4, 4), dtype=np.int32))
    inf = img.copy()
    inf[5, 5] = np.inf  # the plain route has no finiteness test: +inf is a bright pixel
    assert np.array_equal(objmask.apply_object_mask(inf)[1], R.apply_object_mask(inf)[1]) and objmask.apply_object_mask(inf)[1][5, 5]


def test_jwst_valid():
    import torch

    from pyimcom_amd import objmask

    img = R.scene((40, 50), np.float32, 30, nonfinite=6)
    perm = np.random.default_rng(1).uniform(size=img.shape) > 0.1
    valid = ~np.isnan(img)
    got_img, got_mask = objmask.jwst_valid(torch.as_tensor(img, device=DEV), torch.as_tensor(perm, device=DEV))
    assert got_img.is_cuda and same(got_img.cpu().numpy(), np.where(valid, img, 0.0).astype(np.float32))
    assert np.array_equal(got_mask.cpu().numpy(), np.logical_and(perm, valid))
    host_img, host_mask = objmask.jwst_valid(img, perm)
    assert np.array_equal(host_img, np.where(valid, img, 0.0)) and np.array_equal(host_mask, np.logical_and(perm, valid))


# ---- the engine ----
def _engine(z, coords, images, masks, object_mask=None):
    from pyimcom_amd import destripe

    nside = int(z["nside"])
    eng = destripe.DestripeEngine(nside, nside)
    for k in range(int(z["n_sca"])):
        if object_mask is None:
            eng.add_sca(images[k], masks[k], z["g_eff"][k])
        else:
            eng.add_sca(images[k], masks[k], z["g_eff"][k], object_mask=object_mask)
    for a, b in sorted(coords):
        eng.set_pair(a, b, x=coords[(a, b)][0], y=coords[(a, b)][1])
    return eng


def _with_a_star(z, dtype):
    """The mosaic's images, each with one bright star on top (a different place in each), in ``dtype``."""
    yy, xx = np.mgrid[:int(z["nside"]), :int(z["nside"])]
    return [(z["image"][k] + 400.0 * np.exp(-((yy - 15 - 12 * k) ** 2 + (xx - 40 + 9 * k) ** 2) / 8.0)).astype(dtype) for k in range(int(z["n_sca"]))]


@pytest.mark.parametrize("pars", [(0, 0.3, "fits"), (1.05, 0.3, "fits"), (0, 12.0, "jwst")], ids=["issue", "fits", "jwst"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_engine_object_mask_equals_the_mask_made_on_the_host(pars, dtype):
    z, _, coords, _, _ = load_case(GOLDEN[0])
    n = int(z["n_sca"])
    images = _with_a_star(z, dtype)
    host = [R.apply_object_mask(images[k], threshold_m=pars[0], threshold_c=pars[1], type=pars[2])[1] for k in range(n)]
    if pars != (0, 0.3, "fits"):  # (with the issue's thresholds every pixel of these images, near 100, is bright)
        assert all(0 < np.count_nonzero(h) < h.size for h in host[1:])  # (SCA 0 holds a NaN: the plain route masks nothing there)
    want = _engine(z, coords, images, [z["mask"][k] & ~host[k] for k in range(n)])
    got = _engine(z, coords, images, [z["mask"][k] for k in range(n)], object_mask=pars)
    assert "objmask_setup" in got.plan() and "objmask_setup" not in want.plan()
    assert got.plan()["total"] == want.plan()["total"] + got.plan()["objmask_setup"]
    assert got.N_eff.cpu().numpy().tobytes() == want.N_eff.cpu().numpy().tobytes()
    assert "objmask_setup" not in got.plan()  # a peak of the set-up, gone with it
    assert got._frozen["mask"].cpu().numpy().tobytes() == want._frozen["mask"].cpu().numpy().tobytes()
    assert got._frozen["image"].cpu().numpy().tobytes() == want._frozen["image"].cpu().numpy().tobytes()  # not zeroed
    e1, psi1 = got.cost(z["params"], "quadratic")
    e2, psi2 = want.cost(z["params"], "quadratic")
    assert e1 == e2 and psi1.cpu().numpy().tobytes() == psi2.cpu().numpy().tobytes()
    assert got.residual(psi1, "quadratic").tobytes() == want.residual(psi2, "quadratic").tobytes()


def test_flag_entries_with_host_arrays():
    """The staged (host memspace) side of the flag, propagation and apply entries, which the module itself never takes."""
    from pyimcom_amd import _lib

    ctx, L = _lib.default_context(), _lib.lib
    img = G["jwst_f32__image"]
    n, (H, W) = img.size, img.shape
    bkg, ts, tg = float(G["jwst_f32__bkg"]), float(G["jwst_f32__seed_threshold"]), float(G["jwst_f32__grow_threshold"])
    seed, grow, keep = (np.zeros((H, W), dtype=np.uint8) for _ in range(3))
    count = np.zeros(1, dtype=np.int64)
    assert L.imcom_mask_threshold(ctx.handle, _lib.ptr(img), 0, n, bkg, ts, tg, 1, _lib.ptr(seed), _lib.ptr(grow), _lib.MEM_HOST) == 0
    assert np.array_equal(seed.view(np.bool_), G["jwst_f32__seed_mask"]) and np.array_equal(grow.view(np.bool_), G["jwst_f32__grow_candidates"])
    assert L.imcom_mask_clip(ctx.handle, _lib.ptr(img), 0, n, None, 0.0, 0.0, _lib.ptr(keep), _lib.ptr(count), _lib.MEM_HOST) == 0
    assert np.array_equal(keep.view(np.bool_), np.isfinite(img)) and count[0] == np.isfinite(img).sum()
    assert L.imcom_mask_clip(ctx.handle, _lib.ptr(img), 0, n, _lib.ptr(keep), bkg, float(np.float32(0.1)), _lib.ptr(keep), _lib.ptr(count), _lib.MEM_HOST) == 0
    with np.errstate(invalid="ignore"):
        inside = np.isfinite(img) & (np.abs(img - np.float32(bkg)) < np.float32(0.1))
    assert np.array_equal(keep.view(np.bool_), inside) and count[0] == inside.sum()
    out, sweeps = np.zeros((H, W), dtype=np.uint8), C.c_long(0)
    assert L.imcom_mask_propagate(ctx.handle, _lib.ptr(seed), _lib.ptr(grow), H, W, _lib.ptr(out), C.byref(sweeps), _lib.MEM_HOST) == 0
    assert np.array_equal(out.view(np.bool_), G["jwst_f32__grown_mask"]) and sweeps.value >= 2 and sweeps.value % 2 == 0
    res = np.zeros_like(img)
    mask = np.ascontiguousarray(G["jwst_f32__neighbor_mask"]).view(np.uint8)
    assert L.imcom_mask_apply(ctx.handle, _lib.ptr(img), 0, _lib.ptr(mask), n, _lib.ptr(res), _lib.MEM_HOST) == 0
    assert same(res, G["jwst_f32__image_out"])
    assert L.imcom_mask_apply(ctx.handle, _lib.ptr(img), 3, _lib.ptr(mask), n, _lib.ptr(res), _lib.MEM_HOST) == -1
    assert L.imcom_mask_propagate(ctx.handle, _lib.ptr(seed), _lib.ptr(grow), 0, W, _lib.ptr(out), None, _lib.MEM_HOST) == -1
