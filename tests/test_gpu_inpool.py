"""Seam 17 on the GPU: pyimcom_amd.inpool against tests/golden/inpool.npz, which the reference's own statements wrote from numpy's WCS chain.

Indices, counts, relevance, exposure indices, offsets and data are compared with ==: the golden's generator asserts that every position it
decides on lies more than 1e-6 pixel from a decision boundary, and the device's positions are within 1e-9 of the golden's (seam 16).  Positions
are compared bit for bit with what imcom_wcs_pix2pix returns for the same integer pixels, and on the golden's samples with the 40-digit values
under seam 16's bound of 10 ref_err.  Agreement with astropy is inherited from seam 16 and still unchecked."""

import json
import os

import numpy as np
import pytest

from tests import inpool_reference as P
from tests import wcs_reference as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(ROOT, "tests", "golden", "inpool.npz"))
META = json.loads(str(G["meta"]))
NSIDE, N2, N1P, NF = META["nside"], META["n2"], META["n1P"], META["n_inframe"]
NST = N1P + 2
VARIANTS = [(name, name + suffix, suffix == "" and info["masked"]) for name, info in META["images"].items()
            for suffix in (("", "_nomask") if info["masked"] else ("",))]
_CACHE = {}


def in_wcs(name):
    from pyimcom_amd import wcs as W

    w = W.DeviceWCS.from_header(META["images"][name]["header"], array_shape=(NSIDE, NSIDE))
    assert np.array_equal(w.descriptor, G[f"{name}_desc"])
    return w


def out_wcs():
    from pyimcom_amd import wcs as W

    w = W.DeviceWCS.from_header(META["out_header"], array_shape=(N1P * N2, N1P * N2))
    assert np.array_equal(w.descriptor, G["out_desc"])
    return w


def npixmax():
    from pyimcom_amd import inpool

    return inpool.npixmax_of(N2, META["dtheta_deg"])


def partition(name, masked, **kw):
    from pyimcom_amd import inpool

    return inpool.partition_image(in_wcs(name), out_wcs(), G["use_instamps"], N2, N1P, kw.pop("npixmax", npixmax()), mask=G[f"{name}_mask"] if masked else None,
                                  sp_res=META["images"][name]["sp_res"], **kw)


def cached(name, key, masked):
    if key not in _CACHE:
        _CACHE[key] = partition(name, masked)
    return _CACHE[key]


def kept(pix_count, width):
    return np.arange(width) < pix_count[..., None]


@pytest.mark.parametrize("name,key,masked", VARIANTS, ids=[v[1] for v in VARIANTS])
def test_indices_counts_and_relevance_equal_the_golden(name, key, masked):
    info = META["images"][name]
    part = cached(name, key, masked)
    assert part.is_relevant == info["is_relevant"]
    assert part.relevant_matrix.dtype == bool and np.array_equal(part.relevant_matrix, G[f"{name}_relevant"]) and np.array_equal(part.sp_arr, G[f"{name}_sp_arr"])
    if not info["is_relevant"]:
        assert part.y_idx is None and part.x_val is None and part.pix_count is None and part.max_count == 0  # nothing allocated
        return
    got = part.numpy()
    assert part.n_visited == info["visits"]
    for k in ("y_idx", "x_idx", "pix_count"):
        assert got[k].dtype == G[f"{key}_{k}"].dtype and np.array_equal(got[k], G[f"{key}_{k}"]), k
    assert part.max_count == int(G[f"{key}_pix_count"].max())


@pytest.mark.parametrize("name,key,masked", [v for v in VARIANTS if META["images"][v[0]]["is_relevant"]], ids=[v[1] for v in VARIANTS if META["images"][v[0]]["is_relevant"]])
def test_positions_are_those_of_wcs_pix2pix_bit_for_bit(name, key, masked):
    from pyimcom_amd import wcs as W

    got = cached(name, key, masked).numpy()
    on = kept(got["pix_count"], got["x_val"].shape[2])
    pts = np.stack((got["x_idx"][on], got["y_idx"][on]), axis=1).astype(np.float64)
    x, y, _, _ = W._pix2pix(in_wcs(name), out_wcs(), points=pts, nside=NSIDE, want="x")
    assert np.array_equal(got["x_val"][on].view(np.uint64), x.cpu().numpy().view(np.uint64))
    assert np.array_equal(got["y_val"][on].view(np.uint64), y.cpu().numpy().view(np.uint64))
    assert not got["x_val"][~on].any() and not got["y_val"][~on].any()  # zero beyond the count, as np.zeros leaves them
    # the golden's sample of kept pixels (drawn from the masked variant, so every variant keeps them) against the 40-digit positions
    if f"{name}_ref_err" in G:
        frame = np.full((2, NSIDE, NSIDE), np.nan)
        frame[0][got["y_idx"][on], got["x_idx"][on]], frame[1][got["y_idx"][on], got["x_idx"][on]] = got["x_val"][on], got["y_val"][on]
        sx, sy = G[f"{name}_sample_in"][:, 0].astype(int), G[f"{name}_sample_in"][:, 1].astype(int)
        there = np.isfinite(frame[0][sy, sx])
        assert there.all() and 100 <= len(sx) <= 2000
        ex, bound = G[f"{name}_sample_mp"], 10 * G[f"{name}_ref_err"]
        ex_err = np.abs(frame[0][sy, sx] - ex[:, 0])[there].max(), np.abs(frame[1][sy, sx] - ex[:, 1])[there].max()
        print(f"{key}: largest distance from the 40-digit positions {ex_err[0]:.3e}, {ex_err[1]:.3e}; bound {bound[0]:.3e}, {bound[1]:.3e}")
        assert ex_err[0] <= bound[0] and ex_err[1] <= bound[1]


@pytest.mark.parametrize("name,key,masked", [v for v in VARIANTS if META["images"][v[0]]["is_relevant"]], ids=[v[1] for v in VARIANTS if META["images"][v[0]]["is_relevant"]])
def test_extracted_layers_equal_the_golden(name, key, masked):
    import torch

    part = cached(name, key, masked)
    for nf, dk in ((NF, "data"), (1, "data1")):
        frames = P.frames(nf, NSIDE, META["images"][name]["no"])
        data = part.extract_layers(frames if nf == 1 else torch.as_tensor(frames, device="cuda:0"))  # numpy in, and a device tensor in
        assert data.dtype == torch.float32 and data.is_cuda and tuple(data.shape) == G[f"{key}_{dk}"].shape
        assert np.array_equal(data.cpu().numpy(), G[f"{key}_{dk}"]), dk


def build_pool():
    from pyimcom_amd import inpool

    if "pool" not in _CACHE:
        pb = inpool.PoolBuilder(out_wcs(), G["use_instamps"], N2, N1P, npixmax(), NF, nside=NSIDE, sp_res=8)
        flags = []
        for name in META["pool"]:
            info = META["images"][name]
            flags.append(pb.add_image(in_wcs(name), P.frames(NF, NSIDE, info["no"]), G[f"{name}_mask"] if info["masked"] else None))
        _CACHE["pool"] = (pb, flags) + pb.finish()
    return _CACHE["pool"]


def test_pool_of_five_images_equals_the_golden_instamps():
    from pyimcom_amd.select import InStampPool

    pb, flags, pool, pix_cumsum = build_pool()
    assert flags == [META["images"][n]["is_relevant"] for n in META["pool"]] == [True, True, False, False, True]
    assert pix_cumsum.dtype == np.uint32 and np.array_equal(pix_cumsum, G["pool_pix_cumsum"])
    assert np.array_equal(pool.inst_off, G["pool_inst_off"]) and np.array_equal(pool.inst_off_dev.cpu().numpy(), G["pool_inst_off"])
    expo, data = pool.expo.cpu().numpy(), pool.data.cpu().numpy()
    assert expo.dtype == np.int32 and np.array_equal(expo, G["pool_expo"]) and set(expo.tolist()) == {0, 1, 2}
    assert data.dtype == np.float32 and np.array_equal(data, G["pool_data"])
    assert pool.n_inst == NST * NST and pool.npool == len(G["pool_x"]) and pool.n_inframe == NF
    # the positions: those of the images partitioned alone, bit for bit, laid out as InStamp.__init__ lays them out ...
    images = []
    for name in META["pool"]:
        info = META["images"][name]
        if info["is_relevant"]:
            d = cached(name, name, info["masked"]).numpy()
            d["data"] = G[f"{name}_data"]
            images.append(d)
    stamps, cum = P.instamps(images, NF)
    assert np.array_equal(cum, pix_cumsum)
    x, y = pool.x.cpu().numpy(), pool.y.cpu().numpy()
    ref = P.pool_arrays(stamps)
    assert np.array_equal(x.view(np.uint64), ref[0].view(np.uint64)) and np.array_equal(y.view(np.uint64), ref[1].view(np.uint64))
    # ... and the pool that InStampPool.__init__ makes of the same InStamps holds the same five arrays
    host = InStampPool(stamps, NF)
    for k in ("x", "y", "data", "expo", "inst_off_dev"):
        assert np.array_equal(getattr(host, k).cpu().numpy(), getattr(pool, k).cpu().numpy()), k
    assert np.array_equal(host.inst_off, pool.inst_off) and host.n_inst == pool.n_inst and host.npool == pool.npool
    # against the golden's own positions (numpy's chain through (ra, dec)): |device - exact| <= 10 ref_err, |golden - exact| <= ref_err
    bound = 11 * max(G["a_ref_err"].max(), G["b_ref_err"].max())
    err = max(np.abs(x - G["pool_x"]).max(), np.abs(y - G["pool_y"]).max())
    print(f"pool positions: largest distance from the golden's {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_two_runs_and_the_builder_give_the_same_bits():
    first, second = cached("a", "a", True).numpy(), partition("a", True).numpy()
    for k in ("y_idx", "x_idx", "y_val", "x_val", "pix_count"):
        assert np.array_equal(first[k].view(np.uint8), second[k].view(np.uint8)), k
    pb = build_pool()[0]
    on = kept(first["pix_count"], first["x_val"].shape[2])
    x, y, data = (t.cpu().numpy() for t in pb.lists[0])  # image a's compact stamp-major lists inside the builder
    assert np.array_equal(x.view(np.uint64), first["x_val"][on].view(np.uint64)) and np.array_equal(y.view(np.uint64), first["y_val"][on].view(np.uint64))
    assert np.array_equal(pb.counts[0], first["pix_count"].ravel())
    assert data.shape == (NF, on.sum()) and np.array_equal(data, G["a_data"][:, kept(first["pix_count"], G["a_data"].shape[3])])


def test_npixmax_one_below_the_fullest_stamp_is_refused():
    from pyimcom_amd._lib import ImcomError

    full = int(G["a_nomask_pix_count"].max())
    assert partition("a", False, npixmax=full).max_count == full
    with pytest.raises(ImcomError, match=f"more than npixmax={full - 1}"):
        partition("a", False, npixmax=full - 1)


def test_mask_as_a_device_tensor_of_uint8():
    import torch

    from pyimcom_amd import inpool

    mask = torch.as_tensor(G["a_mask"].view(np.uint8), device="cuda:0")  # the form simmask returns with device_out
    part = inpool.partition_image(in_wcs("a"), out_wcs(), G["use_instamps"], N2, N1P, npixmax(), mask=mask, sp_res=8)
    ref = cached("a", "a", True).numpy()
    got = part.numpy()
    for k in ("y_idx", "x_idx", "y_val", "x_val", "pix_count"):
        assert np.array_equal(got[k].view(np.uint8), ref[k].view(np.uint8)), k


def test_fused_equals_composed_at_full_size():
    """One 4088^2 TAN-SIP image with a float32 error table and niter 3 against a block that covers about a quarter of it: the fused launch
    equals select.partition_pixels fed wcs._pix2pix positions in select.visiting_order -- the path of the parent commit -- in all five arrays,
    and extract_layers equals numpy's fancy indexing on the same indices."""
    import torch

    from pyimcom_amd import inpool, select
    from pyimcom_amd import wcs as W
    from tests.golden.make_golden_wcs import _header, _rot, _sip

    nside, n2, n1P = 4088, 32, 24
    nst = n1P + 2
    scale = 0.27 / 3600.0  # 26 stamps of 32 output pixels span 2042 input pixels
    rng = np.random.default_rng(5)
    # a smooth error map of 512 nodes; beyond them the table's end cells extrapolate it over the rest of the chip (noise in the map would be
    # amplified n_pad / a times there and stretch the pixel scale)
    yy, xx = np.mgrid[0:512, 0:512] / 512.0
    errmap = np.stack((0.04 * np.sin(3.1 * xx + 1.3 * yy), 0.03 * np.cos(2.2 * yy - 0.7 * xx)))
    table = W.error_table(errmap, a=8, n_pad=3600, use_float32=True)
    a = W.DeviceWCS.from_header(_header("TAN-SIP", 53.1, -40.0, _rot(0.11 / 3600.0, 30.0, 1), 2044.5, _sip(4, 3, 3, 2044.0)), array_shape=(nside, nside), table=table, niter=3)
    ra, dec = R.np_pix2world(a.descriptor, table, np.array([1022.0]), np.array([1022.0]), 0)  # the block's centre: the middle of the image's first quadrant
    b = W.DeviceWCS.from_header(_header("STG", float(ra[0]), float(dec[0]), _rot(scale, 0.0, 1), n1P * n2 / 2 + 0.5), array_shape=(n1P * n2, n1P * n2))
    use = np.ones((nst, nst), dtype=bool)
    use[5, 7] = use[0, 0] = False
    mask = rng.uniform(size=(nside, nside)) > 0.02
    npixmax = inpool.npixmax_of(n2, scale)
    part = inpool.partition_image(a, b, use, n2, n1P, npixmax, mask=mask)
    assert part.is_relevant and 0.15 < part.relevant_matrix.mean() < 0.6
    total = int(part.pix_count_host.sum())
    print(f"visited {part.n_visited} pixels, kept {total}, fullest stamp {part.max_count} of npixmax {npixmax}")
    assert 0.15 * nside ** 2 < total < 0.3 * nside ** 2
    # composed
    vy, vx = select.visiting_order(part.relevant_matrix, part.sp_arr)
    assert len(vy) == part.n_visited
    ox, oy, _, _ = W._pix2pix(a, b, points=np.stack((vx, vy), axis=1).astype(np.float64), nside=nside, want="x")
    ref = select.partition_pixels(ox, oy, vx, vy, mask[vy, vx], use, n2, n1P, npixmax)
    for got, want, k in zip((part.y_idx, part.x_idx, part.y_val, part.x_val, part.pix_count), ref, ("y_idx", "x_idx", "y_val", "x_val", "pix_count")):
        assert got.dtype == want.dtype and torch.equal(got.view(torch.uint8), want.view(torch.uint8)), k
    # extract_layers
    indata = rng.integers(0, 1 << 20, size=(2, nside, nside)).astype(np.float32)
    data = part.extract_layers(indata).cpu().numpy()
    y_idx, x_idx = part.y_idx.cpu().numpy()[..., :part.max_count], part.x_idx.cpu().numpy()[..., :part.max_count]
    want = np.where(kept(part.pix_count_host, part.max_count)[None], indata[:, y_idx, x_idx], np.float32(0))
    assert data.shape == want.shape and np.array_equal(data, want)


def test_block_seam_reads_an_adopted_pool(golden):
    """The route PoolBuilder -> refblock: with ``blk.instamp_pool`` (a pool adopted by InStampPool.from_device) and InStamps that carry only what
    the host still reads, the block seam writes the bits it writes from the reference's InStamps."""
    import torch

    from pyimcom_amd.refblock import coadd_output_stamps
    from pyimcom_amd.select import InStampPool
    from tests.test_gpu_refblock import Empty, reference_block

    g = golden("stamp_chain")
    stamps = [(int(g["j_st"]), int(g["i_st"]))]
    blk, psfgrp = reference_block(g)
    coadd_output_stamps(blk, psfgrp, flat_penalty=float(g["flat_penalty"]), stamps=stamps, finalize=False, batch=4)
    blk2, _ = reference_block(g)
    x, y, data, expo, off = P.pool_arrays([(st.x_val, st.y_val, st.data, st.pix_cumsum) for row in blk2.instamps for st in row])
    dev = torch.device("cuda:0")
    blk2.instamp_pool = InStampPool.from_device(*(torch.as_tensor(np.ascontiguousarray(v), device=dev) for v in (x, y, data, expo, off)), blk2.cfg.n_inframe)
    for row in blk2.instamps:
        for k, st in enumerate(row):
            lean = Empty()
            lean.pix_cumsum, lean.pix_count = st.pix_cumsum, st.pix_count
            if hasattr(st, "psf_compute_point_pix"):
                lean.psf_compute_point_pix = st.psf_compute_point_pix
            row[k] = lean
    coadd_output_stamps(blk2, psfgrp, flat_penalty=float(g["flat_penalty"]), stamps=stamps, finalize=False, batch=4)
    for k in ("out_map", "UC_map", "Sigma_map", "kappa_map", "Tsum_map", "Neff_map", "T_weightmap"):
        assert np.array_equal(getattr(blk, k), getattr(blk2, k)), k
    assert np.abs(blk.out_map).max() > 0


def test_attach_hands_the_block_what_the_seam_reads():
    pb = build_pool()[0]
    blk = type("Blk", (), {})()
    pool = pb.attach(blk)
    assert blk.instamp_pool is pool and blk.n_inimage == 3 and len(blk.instamps) == NST and pool.n_inst == NST * NST
    cum = np.array([st.pix_cumsum for row in blk.instamps for st in row])
    assert np.array_equal(cum, G["pool_pix_cumsum"]) and np.array_equal(blk.instamps[2][3].pix_count, np.diff(G["pool_pix_cumsum"][2 * NST + 3].astype(np.int64)))
    assert blk.instamps[2][4].psf_compute_point_pix == [4 * N2 - 0.5, 2 * N2 - 0.5] and not hasattr(blk.instamps[2][3], "psf_compute_point_pix")
