"""pyimcom_amd.i24 on the device (csrc/i24.hip) against the reference's own outputs (tests/golden/i24.npz) and, for inputs beyond the
fixtures, against the numpy restatement that tests/test_i24_host.py pins to them.  Every comparison is == on integers and on float32 bit
patterns.  The tile sizes come from csrc/i24_core.h through ``i24.tile_constants()``."""

import numpy as np
import pytest

from tests import i24_reference as R
from tests.test_i24_host import FOREIGN, NAMES, G, bits, pars_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BITKEEPS = [7, 8, 9, 16, 17, 20, 23, None]
DOC = {"VMIN": -0.5, "VMAX": 1.5, "BITKEEP": 20, "DIFF": True, "SOFTBIAS": -1}  # the documented call (docs/compress_README.rst)


def with_bitkeep(pars, bk):
    pars = {k: v for k, v in pars.items() if k != "BITKEEP"}
    if bk is not None:
        pars["BITKEEP"] = bk
    return pars


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def table(ov):
    return ov.columns()


def round_trip(im, scheme, pars):
    """The restatement's decompress(compress(im))."""
    data, tab = R.compress(im, scheme, pars)
    return R.decompress(data, scheme, pars, tab)


def check_against(im, pars, want=None):
    """Both schemes and both directions of one image on the device against ``want`` (A, B, (oy, ox, ov), decA, decB) or the restatement."""
    from pyimcom_amd import i24

    if want is None:
        a, tab = R.compress(im, "I24A", pars)
        b, _ = R.compress(im, "I24B", pars)
        dec = R.decompress(a, "I24A", pars, tab)
        want = (a, b, tab, dec, dec)
    a, ova = i24.i24compress(im, "I24A", pars)
    b, ovb = i24.i24compress(im, "I24B", pars)
    assert same(a, want[0]), "I24A codes"
    assert same(b, want[1]), "I24B cube"
    for ov in (ova, ovb):
        got = table(ov)
        assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.float32
        assert all(same(g, w.astype(g.dtype)) for g, w in zip(got, want[2])), "overflow table"
    assert same(i24.i24decompress(a, "I24A", pars, overflow=ova), want[3]), "decompressed I24A"
    assert same(i24.i24decompress(b, "I24B", pars, overflow=ovb), want[4]), "decompressed I24B"
    return a, b, ova


@pytest.mark.parametrize("name", NAMES)
def test_fixture_cases(name):
    g = lambda k: G[f"{name}/{k}"]  # noqa: E731
    check_against(g("in"), pars_of(name), (g("A"), g("B"), (g("oy"), g("ox"), g("ov")), g("decA"), g("decB")))


@pytest.mark.parametrize("name", FOREIGN)
def test_hand_made_inputs_of_the_decompression(name):
    """A foreign cube with bits above BITKEEP goes through the reference's integer arithmetic unmasked; an I24A image of all 2^BITKEEP - 1
    under DIFF."""
    from pyimcom_amd import i24

    im = G[f"{name}/in"]
    assert same(i24.i24decompress(im, "I24B" if im.dtype == np.uint8 else "I24A", pars_of(name)), G[f"{name}/dec"])


@pytest.mark.parametrize("bk", BITKEEPS)
def test_every_byte_edge_at_more_than_one_tile(bk):
    """33 x 65 (two tiles, n odd) and 300 x 301 (45 tiles, n = 4 mod 8), REORDER on and off, at every BITKEEP of the list."""
    rng = np.random.default_rng(100 + (bk or 24))
    for shape in ((33, 65), (300, 301)):
        im = rng.normal(0.5, 0.6, shape).astype(np.float32)
        for reorder in (True, False):
            check_against(im, with_bitkeep(dict(DOC, REORDER=reorder), bk))


def tile_shapes():
    from pyimcom_amd import i24

    tile, chunk = i24.tile_constants()
    assert tile % 64 == 0
    big = (2 * chunk + 1) * tile + 5  # the scan of the tile sums takes three steps, the last of one sum
    return tile, [(tile // 64 - 1, 64), (1, tile - 1), (tile // 64, 64), (1, tile + 1), (3, tile), (1, big)]


def test_tile_edges_and_the_scan_of_tile_sums():
    tile, shapes = tile_shapes()
    rng = np.random.default_rng(7)
    for shape in shapes:
        n = shape[0] * shape[1]
        im = rng.normal(0.5, 0.45, shape).astype(np.float32)
        flat = im.reshape(-1)
        flat[np.abs(flat - 0.5) > 1.0] = 0.5  # no overflow but the ones placed here
        for p in (0, tile - 1, tile, n - 1):  # the first, two on either side of a tile edge, the last
            if p < n:
                flat[p] = 9.0 + p
        a, b, ov = check_against(im, DOC)
        assert len(ov) == len({p for p in (0, tile - 1, tile, n - 1) if p < n})
        check_against(im, {"VMIN": -0.5, "VMAX": 1.5, "BITKEEP": 9, "DIFF": True, "SOFTBIAS": 64})


def test_prefix_sum_wraps_2_to_the_32():
    """An I24A image of all 2^BITKEEP - 1 under DIFF: the running sum passes 2^32 within the first tile and many times after."""
    from pyimcom_amd import i24

    tile, _ = i24.tile_constants()
    for bk in (23, None, 7):
        pars = with_bitkeep({"VMIN": 0.0, "VMAX": 1.0, "DIFF": True}, bk)
        q = np.full((3, tile + 5), 2 ** (bk or 24) - 1, dtype=np.int32)
        assert int(q.astype(np.int64).sum()) > 2**32 or bk == 7
        assert same(i24.i24decompress(q, "I24A", pars), R.decompress(q, "I24A", pars))
        assert same(i24.i24decompress(q, "I24A", dict(pars, SOFTBIAS=-1)), R.decompress(q, "I24A", dict(pars, SOFTBIAS=-1)))


@pytest.mark.parametrize("kind", ["none", "all", "first", "last", "edges", "nonfinite"])
def test_overflow_tables(kind):
    rng = np.random.default_rng(3)
    im = rng.uniform(0.2, 0.6, (37, 65)).astype(np.float32)  # 2405 pixels: two tiles
    lo, hi = np.float32(0.1), np.float32(0.7)
    flat = im.reshape(-1)
    if kind == "all":
        flat[:] = np.where(rng.random(flat.size) < 0.5, rng.uniform(-5, 0.09, flat.size), rng.uniform(0.71, 5, flat.size)).astype(np.float32)
    elif kind == "first":
        flat[0] = -1.0
    elif kind == "last":
        flat[-1] = 2.0
    elif kind == "edges":
        flat[5:11] = [lo, hi, np.nextafter(lo, np.float32(-1)), np.nextafter(hi, np.float32(1)), np.nextafter(lo, np.float32(1)), np.nextafter(hi, np.float32(0))]
    elif kind == "nonfinite":
        flat[[3, 70, 2100, 2404]] = [np.nan, np.inf, -np.inf, np.nan]
    pars = {"VMIN": 0.1, "VMAX": 0.7, "BITKEEP": 17, "DIFF": True}  # 0.1 and 0.7 are no float32 numbers
    _, _, ov = check_against(im, pars)
    assert len(ov) == {"none": 0, "all": flat.size, "first": 1, "last": 1, "edges": 2, "nonfinite": 2}[kind]


def test_a_table_position_outside_the_image_is_refused_and_nothing_breaks():
    from pyimcom_amd import _lib, i24

    im = G["s33x65_p1/in"]
    pars = pars_of("s33x65_p1")
    b, ov = i24.i24compress(im, "I24B", pars)
    y, x, v = ov.columns()
    for bad_y, bad_x in ((33, 0), (0, 65), (-1, 0), (0, -1), (2**31 + 1, 0), (2**40, 3)):
        t = i24.OverflowTable(np.append(y.astype(np.int64), bad_y), np.append(x.astype(np.int64), bad_x), np.append(v, np.float32(1.0)))
        with pytest.raises(_lib.ImcomError, match="outside") as e:
            i24.i24decompress(b, "I24B", pars, overflow=t)
        assert e.value.status == -1
    assert same(i24.i24decompress(b, "I24B", pars, overflow=ov), G["s33x65_p1/decB"])  # the process is healthy


def test_diff_images():
    yy, xx = np.mgrid[0:37, 0:65]
    pars = {"VMIN": -1.0, "VMAX": 1.0, "DIFF": True, "SOFTBIAS": -1}
    for bk in (20, None):
        check_against(np.where((yy * 65 + xx) % 2, 1.0, -1.0).astype(np.float32), with_bitkeep(pars, bk))  # the largest wrap
        check_against(np.full((37, 65), 0.25, dtype=np.float32), with_bitkeep(pars, bk))
        check_against(((yy * 65 + xx) / (37 * 65.0) * 2 - 1).astype(np.float32), with_bitkeep(pars, bk))  # a ramp across row ends


@pytest.mark.parametrize("bk", [17, None])
def test_softbias_kinds(bk):
    im = np.random.default_rng(5).normal(0.5, 0.6, (33, 65)).astype(np.float32)
    for s in (0, 64, 2 ** (bk or 24) - 1, -1, -2):
        for diff in (False, True):
            check_against(im, with_bitkeep({"VMIN": -0.5, "VMAX": 1.5, "SOFTBIAS": s, "DIFF": diff}, bk))


def test_a_crop_of_a_larger_device_tensor_is_read_in_place():
    import torch

    from pyimcom_amd import i24

    big = np.random.default_rng(8).normal(0.5, 0.6, (3, 70, 90)).astype(np.float32)
    t = torch.as_tensor(big, device=DEV)
    view = t[:, 3:68, 11:80]
    assert not view.is_contiguous()
    cubes, ovs = i24.compress_layers(view, [DOC] * 3)
    for l in range(3):
        want, tab = R.compress(np.ascontiguousarray(big[l, 3:68, 11:80]), "I24B", DOC)
        assert same(cubes[l].cpu().numpy(), want) and all(same(g, w) for g, w in zip(ovs[l].columns(), tab))
    d, ov = i24.i24compress(view[1], "I24B", DOC)
    assert d.is_cuda and ov.data["y"].is_cuda and same(d.cpu().numpy(), cubes[1].cpu().numpy())


def test_a_batch_with_different_parameters_equals_the_layers_one_at_a_time():
    import torch

    from pyimcom_amd import i24

    rng = np.random.default_rng(9)
    frames = rng.normal(0.5, 0.7, (5, 45, 47)).astype(np.float32)
    pars = [DOC, {"VMIN": 0.0, "VMAX": 1.0, "BITKEEP": 7, "REORDER": False}, {"VMIN": -0.5, "VMAX": 1.5}, {"VMIN": 0.1, "VMAX": 0.7, "BITKEEP": 9, "SOFTBIAS": 64},
            {"VMIN": -2.0, "VMAX": 3.0, "BITKEEP": 16, "DIFF": True}]
    for scheme in ("I24B", "I24A"):
        cubes, ovs = i24.compress_layers(torch.as_tensor(frames, device=DEV), pars, scheme)
        for l in range(5):
            one, ov1 = i24.i24compress(frames[l], scheme, pars[l])
            want, tab = R.compress(frames[l], scheme, pars[l])
            assert same(cubes[l].cpu().numpy(), one) and same(one, want)
            assert all(same(g, w) and same(h, w) for g, h, w in zip(ovs[l].columns(), ov1.columns(), tab))
        back = i24.decompress_layers(cubes, pars, ovs)  # (cubes of 1, 2 and 3 planes: one call each)
        assert back.is_cuda and back.dtype == torch.float32 and tuple(back.shape) == (5, 45, 47)
        for l in range(5):
            assert same(back[l].cpu().numpy(), round_trip(frames[l], scheme, pars[l]))


def test_block_maps_compress_layers():
    import torch

    from pyimcom_amd import i24
    from pyimcom_amd.block import BlockMaps

    bm = BlockMaps(2, 8, 2, 4, 1)
    assert bm.nside == 20
    vals = np.random.default_rng(10).normal(0.5, 0.6, (1, 4, 20, 20)).astype(np.float32)
    bm._out_map.copy_(torch.as_tensor(vals))
    pars = [DOC, {"VMIN": -0.5, "VMAX": 1.5, "BITKEEP": 9}, {"VMIN": 0.0, "VMAX": 1.0}]
    for idx in ([1, 2, 3], [3, 1, 2], [1, 3]):
        cubes, ovs = bm.compress_layers(idx, pars[: len(idx)], fk=2)
        for k, i in enumerate(idx):
            crop = np.ascontiguousarray(vals[0, i, 2:18, 2:18])
            want, ov = i24.i24compress(crop, "I24B", pars[k])
            assert same(cubes[k].cpu().numpy(), want) and all(same(g, w) for g, w in zip(ovs[k].columns(), ov.columns()))
    with pytest.raises(ValueError, match="layer 0"):
        bm.compress_layers([0, 1], pars[:2])
    for idx in ([1, 2, 3], [3, 1, 2]):  # one parameter dict too few, on either path
        with pytest.raises(ValueError, match="parameter dicts"):
            bm.compress_layers(idx, pars[:2])


def test_round_trip_feeds_the_report_seams_as_it_is():
    import torch

    from pyimcom_amd import i24
    from pyimcom_amd.noisespec import power_spectrum_2d
    from pyimcom_amd.reportstats import layer_percentiles

    frames = np.random.default_rng(12).normal(0.0, 0.3, (3, 64, 64)).astype(np.float32)
    frames[1, 5, 6], frames[2, 63, 63] = 7.0, -7.0
    pars = [dict(DOC, VMIN=-1.0, VMAX=1.0)] * 3
    want = np.stack([round_trip(f, "I24B", p) for f, p in zip(frames, pars)])
    cubes, ovs = i24.compress_layers(frames, pars)
    got = i24.decompress_layers(cubes, pars, ovs)
    assert same(got.cpu().numpy(), want)
    up = torch.as_tensor(want, device=DEV)
    assert torch.equal(power_spectrum_2d(got, 2.0), power_spectrum_2d(up, 2.0))
    assert same(layer_percentiles({(0, 0): got}, 60, 2, 1), layer_percentiles({(0, 0): up}, 60, 2, 1))


def test_runs_and_kinds_of_input_give_the_same_bits():
    import torch

    from pyimcom_amd import i24

    im = np.random.default_rng(13).normal(0.5, 0.7, (300, 301)).astype(np.float32)
    b1, ov1 = i24.i24compress(im, "I24B", DOC)
    b2, ov2 = i24.i24compress(im, "I24B", DOC)
    b3, ov3 = i24.i24compress(torch.as_tensor(im, device=DEV), "I24B", DOC)
    assert isinstance(b1, np.ndarray) and b3.is_cuda and len(ov1) > 1000
    assert b1.tobytes() == b2.tobytes() == b3.cpu().numpy().tobytes()
    assert all(a.tobytes() == b.tobytes() == c.tobytes() for a, b, c in zip(ov1.columns(), ov2.columns(), ov3.columns()))
    d1 = i24.i24decompress(b1, "I24B", DOC, overflow=ov1)
    d2 = i24.i24decompress(b1, "I24B", DOC, overflow=ov1)
    d3 = i24.i24decompress(b3, "I24B", DOC, overflow=ov3)
    assert isinstance(d1, np.ndarray) and d3.is_cuda and d1.tobytes() == d2.tobytes() == d3.cpu().numpy().tobytes()
    b4, ov4 = i24.i24compress(torch.as_tensor(im), "I24B", DOC)  # a torch tensor on the host: torch tensors on the host
    d4 = i24.i24decompress(b4, "I24B", DOC, overflow=ov4)
    assert not b4.is_cuda and not ov4.data["value"].is_cuda and not d4.is_cuda
    assert b4.numpy().tobytes() == b1.tobytes() and d4.numpy().tobytes() == d1.tobytes()


def test_one_production_size_layer():
    """2688 x 2688, BITKEEP 20, DIFF, SOFTBIAS -1 against the restatement (whose I24A and I24B decompress to the same image)."""
    import torch

    from pyimcom_amd import i24

    n = 2688
    rng = np.random.default_rng(14)
    im = rng.normal(0.5, 0.4, (n, n)).astype(np.float32)
    a, tab = R.compress(im, "I24A", DOC)
    want_b = np.stack([R.stream_fwd(((a >> (8 * j)) & 255).astype(np.uint8)) for j in range(3)])
    want_dec = R.decompress(a, "I24A", DOC, tab)
    cube, ov = i24.i24compress(torch.as_tensor(im, device=DEV), "I24B", DOC)
    assert same(cube.cpu().numpy(), want_b)
    assert len(tab[0]) > 10000 and all(same(g, w) for g, w in zip(ov.columns(), tab))
    assert same(i24.i24decompress(cube, "I24B", DOC, overflow=ov).cpu().numpy(), want_dec)
