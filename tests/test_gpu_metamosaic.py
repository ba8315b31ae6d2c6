"""The device metadetection mosaic (seam 19) on the GPU: pyimcom_amd.metamosaic against tests/golden/metamosaic.npz (the reference's own
statements) and, for the one size above the fixture's, against tests/metamosaic_reference.py.  Everything is compared with ``==``; layers
as bits, NaNs included.  The cap cases keep every tested pixel more than 1e-12 r^2 from the circle and the ``mask_caps`` positions more
than 1e-6 pixel from a box bound or a pixel's membership (tests/golden/make_golden_metamosaic.py refuses the others)."""

import numpy as np
import pytest

from tests import metamosaic_reference as MR
from tests.test_metamosaic_host import CAPS, CFG, ENTRIES, META, MOSAICS, G, bits, blocks_of, cfg_like

pytestmark = pytest.mark.gpu


def host(t):
    return t.cpu().numpy()


def new_mosaic(case, cfg=None):
    from pyimcom_amd import metamosaic as M

    m = M.DeviceMetaMosaic(cfg or cfg_like(), case["ix"], case["iy"], case["nlayer"], np.dtype(case["dtype"]), bbox=case["bbox"], extpix=case["extpix"], stem=META["stem"])
    assert (m.trunc, m.Nside) == (case["trunc"], case["Nside"]) and [list(w) for w in m.windows] == case["windows"]
    return m


def strided_on_device(a):
    """``a`` as a view of a larger device tensor: row and plane strides above the shape, an odd element offset."""
    import torch

    t = torch.as_tensor(a.view(np.int16) if a.dtype == np.uint16 else a)
    big = torch.zeros(tuple(t.shape[:-2]) + (t.shape[-2] + 3, t.shape[-1] + 5), dtype=t.dtype, device="cuda:0")
    view = big[..., 1:1 + t.shape[-2], 3:3 + t.shape[-1]]
    view.copy_(t)
    return view.view(torch.uint16) if a.dtype == np.uint16 else view


def build(case, order=None, source="host"):
    m = new_mosaic(case)
    blocks = blocks_of(case)
    wins = list(m.windows) if order is None else [m.windows[k] for k in order]
    for w in wins:
        b = blocks[(w[2], w[3])]
        arrays = [b["primary"], b["fidelity"], b["sigma"]]
        if source == "device":
            arrays = [strided_on_device(a) for a in arrays]
        m.add_block(w[0], w[1], *arrays, b["fid_bels"], b["sig_bels"])
    return m


def assert_equals_golden(m, name, image=True):
    if image:
        got = host(m.in_image)
        assert got.dtype == G[name + "_image"].dtype and np.array_equal(bits(got), bits(G[name + "_image"]))
    assert np.array_equal(bits(host(m.in_fidelity)), bits(G[name + "_fidelity"])) and np.array_equal(bits(host(m.in_noise)), bits(G[name + "_noise"]))
    assert host(m.in_mask).dtype == bool and np.array_equal(host(m.in_mask), G[name + "_mask"])


@pytest.mark.parametrize("name", sorted(MOSAICS))
def test_mosaic_arrays_equal_the_reference(name):
    m = build(MOSAICS[name])
    assert_equals_golden(m, name)
    image, fid, noise, mask = m.to_host()
    assert mask.dtype == np.uint8 and np.array_equal(mask, G[name + "_mask"]) and np.array_equal(bits(image), bits(G[name + "_image"]))
    assert np.array_equal(bits(fid), bits(G[name + "_fidelity"])) and np.array_equal(bits(noise), bits(G[name + "_noise"]))


@pytest.mark.parametrize("name", ["interior", "ext10", "double", "bytes"])
def test_any_order_and_device_tensors_give_the_same_mosaic(name):
    case = MOSAICS[name]
    n = len(case["windows"])
    assert_equals_golden(build(case, order=list(range(n))[::-1], source="device"), name)
    assert_equals_golden(build(case, order=list(np.random.default_rng(3).permutation(n))), name)


def test_big_endian_arrays_are_taken_as_fits_presents_them():
    case = MOSAICS["ext10"]
    m = new_mosaic(case)
    blocks = blocks_of(case)
    for w in m.windows:
        b = blocks[(w[2], w[3])]
        m.add_block(w[0], w[1], b["primary"].astype(">f4"), b["fidelity"].astype(">u2"), b["sigma"].astype(">i2"), b["fid_bels"], b["sig_bels"])
    assert_equals_golden(m, "ext10")


def test_compressed_layers_are_decoded_on_the_device():
    """BITKEEP absent (24 bits kept).  The fixture's layers hold NaNs, -0.0 and subnormals, which the codec does not keep bit for bit, so
    the image is compared with a mosaic built from the decompressed layers; the maps and the mask do not depend on the layers and equal
    the golden."""
    import torch

    from pyimcom_amd import i24

    case = MOSAICS["interior"]
    pars = [{"VMIN": -4.0, "VMAX": 4.0}] * case["nlayer"]
    a, b = new_mosaic(case), new_mosaic(case)
    survived = total = 0
    for w in a.windows:
        blk = blocks_of(case)[(w[2], w[3])]
        cubes, overflows = i24.compress_layers(blk["primary"], pars)
        a.add_block_compressed(w[0], w[1], cubes, pars, overflows, blk["fidelity"], blk["sigma"], blk["fid_bels"], blk["sig_bels"])
        layers = i24.decompress_layers(cubes, pars, overflows)
        assert layers.is_cuda and layers.dtype == torch.float32
        b.add_block(w[0], w[1], layers, blk["fidelity"], blk["sigma"], blk["fid_bels"], blk["sig_bels"])
        same = bits(host(layers)) == bits(blk["primary"])
        survived, total = survived + int(same.sum()), total + same.size
    print(f"I24 with 24 bits: {survived} of {total} layer values survive bit for bit")
    assert np.array_equal(bits(host(a.in_image)), bits(host(b.in_image))) and host(a.in_image).any()
    assert_equals_golden(a, "interior", image=False)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_large_window_at_an_odd_offset(dtype):
    """2051 x 2048 pixels from (3, 5) of a 2060 x 2061 file to (14, 13) of a mosaic of side 2112: rows whose source and destination agree in
    their offset within 16 bytes take the 16-byte path, the others go element by element; every bit pattern occurs in the layers."""
    import types

    from pyimcom_amd import metamosaic as M

    rng = np.random.default_rng(2048)
    nlayer, by, bx = 2, 2060, 2061
    window = (3, 2054, 5, 2053, 8, 11)  # symin, symax, sxmin, sxmax, cx, cy
    primary = rng.integers(0, 2**32, size=(nlayer, by, bx), dtype=np.uint32).view(np.float32)
    if dtype == "float64":
        primary = rng.integers(0, 2**63, size=(nlayer, by, bx), dtype=np.uint64).view(np.float64)
    fid = rng.integers(0, 2**16, size=(by, bx), dtype=np.uint16)
    sig = rng.integers(-2**15, 2**15, size=(by, bx), dtype=np.int16)
    cfg = types.SimpleNamespace(**dict(CFG, n1=2, n2=352))
    m = M.DeviceMetaMosaic(cfg, 1, 1, nlayer, np.dtype(dtype))
    assert m.Nside == 2112
    m.paste(window, primary, fid, sig, -2e-4, 3e-4)
    want = (np.zeros((nlayer, 2112, 2112), dtype=dtype), np.zeros((2112, 2112), dtype=np.float32), np.zeros((2112, 2112), dtype=np.float32))
    MR.paste(want, window, primary, fid, sig, -2e-4, 3e-4)
    assert np.array_equal(bits(host(m.in_image)), bits(want[0]))
    assert np.array_equal(bits(host(m.in_fidelity)), bits(want[1])) and np.array_equal(bits(host(m.in_noise)), bits(want[2]))
    mask = np.ones((2112, 2112), dtype=bool)
    mask[14:2065, 13:2061] = want[1][14:2065, 13:2061] == 0
    assert np.array_equal(host(m.in_mask), mask) and 0 < (~mask).sum() < 2051 * 2048


def test_mask_methods_equal_the_reference():
    import torch

    m = build(MOSAICS["interior"])
    m.mask_fidelity_cut(META["cuts"]["fidelitymin"])
    assert np.array_equal(host(m.in_mask), G["cut_fidelity"])
    m.mask_noise_cut(META["cuts"]["noisemax"])
    assert np.array_equal(host(m.in_mask), G["cut_noise"])
    before = m.in_mask.clone()
    m.maskpix(G["extramask"])
    assert np.array_equal(host(m.in_mask), G["cut_extra"])
    m.in_mask.copy_(before)
    m.maskpix(torch.as_tensor(G["extramask"]).to("cuda:0"))
    assert np.array_equal(host(m.in_mask), G["cut_extra"])
    # a cut given as float64 is compared in float64, as numpy compares it
    m = build(MOSAICS["interior"])
    cut = np.float64(G["interior_fidelity"][np.isfinite(G["interior_fidelity"])].max()) * (1 - 2.0**-40)
    m.mask_fidelity_cut(cut)
    assert np.array_equal(host(m.in_mask), np.logical_or(G["interior_fidelity"] < cut, G["interior_mask"]))
    with pytest.raises(ValueError):
        m.maskpix(np.zeros((5, 5), dtype=bool))


@pytest.mark.parametrize("name", CAPS)
def test_circles_equal_the_reference(name):
    x, y, r = G[f"caps_{name}_xyr"]
    want = G[f"caps_{name}_mask"]
    m = new_mosaic(MOSAICS["interior"])
    n = len(x)
    perm = np.random.default_rng(11).permutation(n)
    for xs, ys, rs, calls in ((x, y, r, 1), (x[perm], y[perm], r[perm], 1), (x, y, r, 2)):
        m.in_mask.zero_()
        if calls == 1:
            m.mask_caps_pixels(xs, ys, rs)
        else:
            m.mask_caps_pixels(xs[: n // 2], ys[: n // 2], rs[: n // 2])
            m.mask_caps_pixels(xs[n // 2:], ys[n // 2:], rs[n // 2:])
        assert np.array_equal(host(m.in_mask), want), calls
    m.in_mask.fill_(True)  # only ones are written: a masked pixel stays masked
    m.mask_caps_pixels(x, y, r)
    assert bool(m.in_mask.all())


def test_circles_from_device_tensors_and_refusals():
    import torch

    x, y, r = (torch.as_tensor(v).to("cuda:0") for v in G["caps_random_xyr"])
    m = new_mosaic(MOSAICS["interior"])
    m.in_mask.zero_()
    m.mask_caps_pixels(x, y, r)
    assert np.array_equal(host(m.in_mask), G["caps_random_mask"])
    before = m.in_mask.clone()
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError):
            m.mask_caps_pixels([10.0, bad], [10.0, 20.0], [3.0, 3.0])
    with pytest.raises(ValueError):
        m.mask_caps_pixels([10.0, 20.0], [10.0], [3.0, 3.0])
    assert torch.equal(m.in_mask, before)


def test_mask_caps_from_the_catalogue_equals_the_reference():
    m = build(MOSAICS["interior"])
    first = m.in_mask.clone()
    m.mask_caps(G["sky_ra"], G["sky_dec"], G["sky_radius"])
    assert np.array_equal(host(m.in_mask), G["sky_array_mask"])
    m.in_mask.copy_(first)
    m.mask_caps(G["sky_ra"], G["sky_dec"], float(G["sky_scalar_radius"]))
    assert np.array_equal(host(m.in_mask), G["sky_scalar_mask"])
    m.in_mask.copy_(first)
    m.mask_caps(G["sky_ra"][-3:-1], G["sky_dec"][-3:-1], float(G["sky_scalar_radius"]))  # nothing near the mosaic: nothing changes
    assert np.array_equal(host(m.in_mask), G["interior_mask"])


@pytest.mark.parametrize("k", range(len(META["orig"])))
def test_origimage_equals_the_reference(k):
    o = META["orig"][k]
    m = build(MOSAICS[o["mosaic"]])
    if o["raises"]:
        with pytest.raises(ValueError, match="overfills"):
            m.origimage(N=o["N"], select_layers=o["select_layers"])
        return
    im = m.origimage(N=o["N"], select_layers=o["select_layers"])
    assert np.array_equal(bits(host(im["image"])), bits(G[f"orig{k}_image"])) and np.array_equal(host(im["mask"]), G[f"orig{k}_mask"])
    assert MR.plain(im["pars"]) == o["pars"] and list(im["pars"]) == list(o["pars"]) and im["layers"] == o["layers"]
    assert MR.plain(im["ref"]) == o["ref"] and im["psf_fwhm"] == o["psf_fwhm"] and MR.plain(im["wcs"]) == o["header"]
    assert im["device_wcs"].array_shape == G[f"orig{k}_mask"].shape
    if o["select_layers"] is None:
        assert im["image"].data_ptr() >= m.in_image.data_ptr() and im["image"]._base is not None  # a view
    im["mask"].fill_(True)
    assert np.array_equal(host(m.in_mask), G[o["mosaic"] + "_mask"])  # a copy


@pytest.mark.parametrize("k", range(len(META["shear"])))
def test_shearimage_hands_the_references_arguments_to_the_resampler(k, monkeypatch):
    import torch

    from pyimcom_amd import ginterp
    from pyimcom_amd import metamosaic as M

    s = META["shear"][k]
    name = s["name"]
    m = build(MOSAICS["interior"])
    calls = []
    direct = ginterp.MultiInterp

    def recording(*args, **kw):
        calls.append((args, kw))
        return direct(*args, **kw)

    monkeypatch.setattr(M.ginterp, "MultiInterp", recording)
    im = m.shearimage(s["N"], jac=None if s["jac"] is None else np.array(s["jac"]), psfgrow=s["psfgrow"], oversamp=s["oversamp"], fidelity_min=s["fidelity_min"],
                      select_layers=s["select_layers"])
    ((args, kw),) = calls
    assert not kw and len(args) == 8
    layers, inmask, out_size, opos, J, Rsearch, samp, C = args
    assert layers.is_cuda and inmask.is_cuda and np.array_equal(bits(host(layers)), bits(G["interior_image"][s["ul"]]))
    assert np.array_equal(host(inmask), G[f"shear_{name}_inmask"]) and list(out_size) == s["out_size"]
    assert np.array_equal(opos, G[f"shear_{name}_opos"]) and np.array_equal(J, G[f"shear_{name}_J"])
    assert (Rsearch, samp, MR.plain(C)) == (s["Rsearch"], s["samp"], s["C"])
    if s["fidelity_min"] is not None:
        assert G[f"shear_{name}_inmask"].sum() > G["interior_mask"].sum()
    assert np.array_equal(host(m.in_mask), G["interior_mask"])  # (the cut of fidelity_min does not touch the mosaic's mask)
    # the same call on the golden arrays
    image, mask, umax, smax = direct(torch.as_tensor(G["interior_image"][s["ul"]]).to("cuda:0"), torch.as_tensor(G[f"shear_{name}_inmask"]).to("cuda:0"), s["out_size"],
                                     G[f"shear_{name}_opos"], G[f"shear_{name}_J"], s["Rsearch"], s["samp"], s["C"])
    assert np.array_equal(bits(host(im["image"])), bits(host(image))) and np.array_equal(host(im["mask"]), host(mask))
    assert tuple(im["image"].shape) == (len(s["ul"]), s["N"], s["N"]) and im["mask"].dtype == torch.bool
    pars = dict(im["pars"])
    assert list(pars)[:5] == ["STEM", "BLOCKX", "BLOCKY", "UMAX", "SMAX"] and pars.pop("UMAX")[0] == umax and pars.pop("SMAX")[0] == smax
    assert MR.plain(pars) == s["pars"] and im["layers"] == s["layers"] and MR.plain(im["ref"]) == s["ref"] and im["psf_fwhm"] == s["psf_fwhm"]
    assert MR.plain(im["wcs"]) == s["header"] and set(im) == {"image", "mask", "wcs", "device_wcs", "pars", "layers", "psf_fwhm", "ref"}
    w = im["device_wcs"].all_pix2world([[s["ref"][0], s["ref"][1]]], 0)[0]
    assert abs(w[0] - CFG["ra"]) < 1e-9 and abs(w[1] - CFG["dec"]) < 1e-9  # the projection centre is the reference pixel


def test_refusals():
    import torch

    from pyimcom_amd import metamosaic as M

    case = MOSAICS["bbox"]
    m = new_mosaic(case)
    b = blocks_of(case)[(1, 1)]
    with pytest.raises(ValueError, match="not among the blocks"):
        m.add_block(1, 0, b["primary"], b["fidelity"], b["sigma"], b["fid_bels"], b["sig_bels"])  # block (2, 1): outside the bbox
    with pytest.raises(ValueError, match="not among the blocks"):
        m.add_block(2, 0, b["primary"], b["fidelity"], b["sigma"], b["fid_bels"], b["sig_bels"])
    for prim, fid, sig in ((b["primary"].astype(np.float16), b["fidelity"], b["sigma"]), (b["primary"].astype(np.float64), b["fidelity"], b["sigma"]),
                           (b["primary"], b["fidelity"].astype(np.int32), b["sigma"]), (b["primary"], b["fidelity"], b["sigma"].astype(np.float32)),
                           (b["primary"], torch.as_tensor(b["fidelity"].astype(np.int64)), b["sigma"])):
        with pytest.raises(TypeError):
            m.add_block(0, 0, prim, fid, sig, b["fid_bels"], b["sig_bels"])
    with pytest.raises(ValueError):
        m.add_block(0, 0, b["primary"][:, :40], b["fidelity"], b["sigma"], b["fid_bels"], b["sig_bels"])
    with pytest.raises(TypeError):
        M.DeviceMetaMosaic(cfg_like(), 1, 1, 1, np.float16)
    assert not host(m.in_image).any() and host(m.in_mask).all()  # nothing was written
    other = M.DeviceMetaMosaic(dict(CFG, outpsf="AIRYOBSC"), 1, 1, 1, np.float32)
    for call in (lambda: other.shearimage(16), lambda: other.origimage()):
        with pytest.raises(ValueError, match="only works on GAUSSIAN"):
            call()


def test_the_library_refuses_a_window_outside_its_arrays():
    from pyimcom_amd._lib import ImcomError

    case = MOSAICS["interior"]
    m = new_mosaic(case)
    b = blocks_of(case)[(1, 2)]
    for window in ((0, 49, 0, 48, 0, 0), (0, 48, -1, 48, 8, 0), (8, 40, 8, 40, 60, 0), (8, 40, 8, 40, 0, -9), (40, 8, 8, 40, 0, 0)):
        with pytest.raises(ImcomError) as e:
            m.paste(window, b["primary"], b["fidelity"], b["sigma"], b["fid_bels"], b["sig_bels"])
        assert e.value.status == -1
    assert not host(m.in_image).any() and host(m.in_mask).all()


@pytest.mark.parametrize("name", ENTRIES)
def test_null_context_is_refused_through_the_abi(name):
    from tests.test_metamosaic_host import test_null_context_is_refused_before_anything_else as refused

    refused(name)
