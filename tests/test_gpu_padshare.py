"""Padding stamps shared between neighbouring blocks (seam 20) on the GPU: pyimcom_amd.padshare against tests/golden/padshare.npz (the
reference's own statements) and against tests/padshare_reference.py where the fixture holds no recorded answer.

Compared bit for bit (NaN matching NaN, the sign of zero included): PRIMARY, INWEIGHT, INWTFLAT, the codes after a replace call, and every
float32 sum before the encode, under either floor rule.  The codes of an add call are compared exactly with the restatement run with the
device's encode (log10 correctly rounded to float32) and, with the reference's recorded codes, under the condition of tests/test_gpu_block.py:
never more than one count apart and different for at most 1 % of the strip's pixels per map (numpy's float32 log10 is not correctly rounded;
the generator measured 0.02 % on the fixture's own sums).  Since the sums are equal, the allowance covers log10 and nothing else."""

import numpy as np
import pytest

from tests import padshare_reference as PR
from tests import test_padshare_host as H

pytestmark = pytest.mark.gpu

G, META, MOSAIC = H.G, H.META, H.MOSAIC


def host(t):
    return t.cpu().numpy()


def share_block(block, n2, pad, fk):
    from pyimcom_amd import padshare as P

    return P.ShareBlock.from_arrays(block["primary"], block["inweight"], block["idscas"], {k: tuple(v) for k, v in block["maps"].items()}, n2, pad, fk)


def assert_block_equals(sb, want, exact_codes=True, direction=None, strip=None):
    got = sb.to_arrays()
    assert PR.same_bits(got["primary"], want["primary"]) and PR.same_bits(got["inweight"], want["inweight"])
    assert PR.same_bits(got["inwtflat"], PR.inwtflat(want["inweight"])) and list(got["maps"]) == list(want["maps"])
    for n in want["maps"]:
        if exact_codes:
            assert PR.same_bits(got["maps"][n][0], want["maps"][n][0]), n
        else:
            assert H.codes_within_the_allowance(got["maps"][n][0], want["maps"][n][0], direction, strip), n


@pytest.fixture(scope="module")
def device_formula():
    return H.device_formula_mosaic()


def test_mosaic_grid_equals_the_reference(device_formula):
    from pyimcom_amd import padshare as P

    m = MOSAIC
    blocks = [[share_block(b, m["n2"], m["postage_pad"], m["fk"]) for b in row] for row in H.mosaic_blocks("in")]
    P.share_padding_stamps(3, blocks)
    exact, recorded = device_formula[0], H.mosaic_blocks("out")
    for iby in range(3):
        for ibx in range(3):
            assert_block_equals(blocks[iby][ibx], exact[iby][ibx])
            assert_block_equals(blocks[iby][ibx], recorded[iby][ibx], exact_codes=False)


def test_mosaic_by_load_and_save_keeps_the_references_order(device_formula):
    from pyimcom_amd import padshare as P

    m = MOSAIC
    inputs, log, files, alive = H.mosaic_blocks("in"), [], {}, []

    def load(iby, ibx):
        log.append(["load", iby, ibx])
        src = files.get((iby, ibx), inputs[iby][ibx])  # (the vertical pass reads what the horizontal pass saved)
        alive.append((iby, ibx))
        return share_block(src, m["n2"], m["postage_pad"], m["fk"])

    def save(iby, ibx, block):
        log.append(["save", iby, ibx])
        a = block.to_arrays()
        files[(iby, ibx)] = {"primary": a["primary"], "inweight": a["inweight"], "idscas": a["idscas"], "maps": {k: list(v) for k, v in a["maps"].items()}}
        alive.remove((iby, ibx))
        assert len(alive) <= 1  # a saved block is let go: the next load makes two

    P.share_padding_stamps(3, load, save)
    assert log == [s for s in m["order"] if s[0] != "update"] and not alive
    for iby in range(3):
        for ibx in range(3):
            got, want = files[(iby, ibx)], device_formula[0][iby][ibx]
            assert PR.same_bits(got["primary"], want["primary"]) and PR.same_bits(got["inweight"], want["inweight"])
            assert all(PR.same_bits(got["maps"][n][0], want["maps"][n][0]) for n in want["maps"])


def test_mosaic_sums_of_every_call_are_exact(device_formula):
    """The 24 updates of the loop one by one, each from the state the restatement (with the device's encode) reached: every map strip's sums."""
    from pyimcom_amd import padshare as P

    m = MOSAIC
    state = H.mosaic_blocks("in")
    updates = [s for s in PR.share_order(3) if s[0] == "update"]
    for k, step in enumerate(updates):
        (ay, ax), (by, bx) = step[1], step[2]
        mine, theirs = share_block(state[ay][ax], m["n2"], m["postage_pad"], m["fk"]), share_block(state[by][bx], m["n2"], m["postage_pad"], m["fk"])
        sums = {}
        P.update(mine, theirs, step[3], step[4], sums=sums)
        want = PR.update(state[ay][ax], state[by][bx], step[3], step[4], m["n2"], m["postage_pad"], m["fk"], encode=PR.compress_device)
        assert all(PR.same_bits(host(sums[n]), want[n]) and PR.same_bits(host(sums[n]), device_formula[1][k][n]) for n in want), step
        assert_block_equals(mine, state[ay][ax])
        assert_block_equals(theirs, state[by][bx])


@pytest.mark.parametrize("name", H.PAIRS)
def test_pair_cases_equal_the_reference(name):
    from pyimcom_amd import padshare as P

    a, b, c = H.pair_blocks(name)
    for k, (direction, add_mode) in enumerate(c["calls"]):
        mine, theirs = share_block(a, c["n2"], c["postage_pad"], c["fk"]), share_block(b, c["n2"], c["postage_pad"], c["fk"])
        sums = {}
        P.update(mine, theirs, direction, add_mode, sums=sums)
        recorded, recorded_sums = H.pair_expected(name, k, a, c)
        my, _ = PR.strips(direction, c["n1P"] * c["n2"], c["postage_pad"] * c["n2"], c["fk"])
        assert_block_equals(mine, recorded, exact_codes=not add_mode, direction=direction, strip=my)
        assert_block_equals(theirs, b)
        assert list(sums) == list(recorded_sums) and all(PR.same_bits(host(sums[n]), recorded_sums[n]) for n in sums), (direction, add_mode)
        exact = PR.copy_block(a)
        PR.update(exact, PR.copy_block(b), direction, add_mode, c["n2"], c["postage_pad"], c["fk"], encode=PR.compress_device)
        assert_block_equals(mine, exact)
        for zero_floor in (True, False):
            mine, want = share_block(a, c["n2"], c["postage_pad"], c["fk"]), PR.copy_block(a)
            sums = {}
            P.update(mine, theirs, direction, add_mode, zero_floor=zero_floor, sums=sums)
            want_sums = PR.update(want, PR.copy_block(b), direction, add_mode, c["n2"], c["postage_pad"], c["fk"], zero_floor, encode=PR.compress_device)
            assert all(PR.same_bits(host(sums[n]), want_sums[n]) for n in sums), (direction, add_mode, zero_floor)
            assert_block_equals(mine, want)


def test_every_code_decodes_as_numpy_decodes_it():
    """All 65536 codes of the five (unit, dtype) pairs through the kernel's decode (a replace call's sums are the neighbour's decoded
    values), bit for bit against np.power(10.0, codes / coef).astype(np.float32)."""
    import torch

    from pyimcom_amd import padshare as P

    n_out, n1P, n2, pad = 8, 4, 32, 2  # my strip: 8 planes of 128 rows x 64 columns = 65536 pixels
    N = n1P * n2
    maps_mine, maps_theirs, want = {}, {}, {}
    for name, (letter, coef, dtype, unit, comment) in PR.MAPS.items():
        lo, hi = PR.code_range(dtype)
        codes = np.arange(lo, hi + 1).astype(dtype)
        theirs = np.zeros((n_out, N, N), dtype=dtype)
        theirs[:, :, N - 2 * pad * n2:N - pad * n2] = codes.reshape(n_out, N, pad * n2)
        maps_theirs[name] = (theirs, unit, comment)
        maps_mine[name] = (np.full((n_out, N, N), 7, dtype=dtype), unit, comment)
        want[name] = np.power(10.0, codes / (1.0 / PR.unit_to_bels(unit, comment))).astype(np.float32).reshape(n_out, N, pad * n2)
    zeros = np.zeros((n_out, 1, N, N), dtype=np.float32), np.zeros((n_out, 1, n1P, n1P), dtype=np.float32)
    mine = P.ShareBlock.from_arrays(zeros[0], zeros[1], [(1, 1)], maps_mine, n2, pad, 0)
    theirs = P.ShareBlock.from_arrays(zeros[0], zeros[1], [(1, 1)], maps_theirs, n2, pad, 0)
    sums = {}
    P.update(mine, theirs, "left", add_mode=False, zero_floor=False, sums=sums)
    torch.cuda.synchronize()
    differing = {n: int(np.sum(host(sums[n]).view(np.uint32) != want[n].view(np.uint32))) for n in want}
    assert differing == {n: 0 for n in want}, differing
    for n in want:  # ... and every code comes back from the encode
        assert np.array_equal(host(mine.maps[n][0])[:, :, :pad * n2], maps_theirs[n][0][:, :, N - 2 * pad * n2:N - pad * n2]), n


def test_a_second_add_is_the_references_second_call():
    from pyimcom_amd import padshare as P

    a, b, c = H.pair_blocks("fk2")
    mine, theirs, want = share_block(a, c["n2"], c["postage_pad"], c["fk"]), share_block(b, c["n2"], c["postage_pad"], c["fk"]), PR.copy_block(a)
    P.update(mine, theirs, "top", True)
    PR.update(want, PR.copy_block(b), "top", True, c["n2"], c["postage_pad"], c["fk"], encode=PR.compress_device)
    once = PR.copy_block(want)
    P.update(mine, theirs, "top", True)
    PR.update(want, PR.copy_block(b), "top", True, c["n2"], c["postage_pad"], c["fk"], encode=PR.compress_device)
    assert_block_equals(mine, want)
    assert not PR.same_bits(want["primary"], once["primary"]) and not PR.same_bits(want["maps"]["SIGMA"][0], once["maps"]["SIGMA"][0])  # not idempotent


def test_from_block_maps_shares_the_blocks_storage():
    import torch

    from pyimcom_amd import padshare as P
    from pyimcom_amd.block import BlockMaps

    n1P, n2, fk, pad, ids = 4, 4, 1, 1, ([(1, 1), (2, 2)], [(2, 2), (3, 3), (1, 1)])
    gen = torch.Generator(device="cuda:0").manual_seed(20)
    bms, shared, plain = [], [], []
    for idscas in ids:
        bm = BlockMaps(n1P, n2, fk, 2, len(idscas), n_out=2)
        bm._out_map.copy_(torch.randn(bm._out_map.shape, generator=gen, device="cuda:0"))
        for k, t in bm._maps.items():
            t.copy_(torch.rand(t.shape, generator=gen, device="cuda:0") * 3 + 0.01)
        bm._maps["Neff"][:, 3:9, 2:7] = 1e-40  # uncovered: the floor code
        bm.T_weightmap.copy_(torch.rand(bm.T_weightmap.shape, generator=gen, device="cuda:0"))
        sb = P.ShareBlock.from_block_maps(bm, fk, idscas, postage_pad=pad)
        assert list(sb.maps) == list(PR.MAPS) and all(sb.maps[n][1:] == (PR.MAPS[n][3], PR.MAPS[n][4]) for n in PR.MAPS)
        assert sb.primary.data_ptr() == bm.out_map[:, :, fk:, fk:].data_ptr() and sb.inweight.data_ptr() == bm.T_weightmap.data_ptr()
        a = sb.to_arrays()
        plain.append(P.ShareBlock.from_arrays(a["primary"], a["inweight"], idscas, a["maps"], n2, pad, fk))
        bms.append(bm)
        shared.append(sb)
    ring = host(bms[0].out_map).copy()
    for direction, add_mode in (("right", True), ("bottom", False)):
        P.update(shared[0], shared[1], direction, add_mode)
        P.update(plain[0], plain[1], direction, add_mode)
    got, want = shared[0].to_arrays(), plain[0].to_arrays()
    assert PR.same_bits(got["primary"], want["primary"]) and PR.same_bits(got["inweight"], want["inweight"]) and PR.same_bits(got["inwtflat"], want["inwtflat"])
    assert all(PR.same_bits(got["maps"][n][0], want["maps"][n][0]) for n in want["maps"])
    now = host(bms[0].out_map)
    assert PR.same_bits(now[:, :, fk:-fk, fk:-fk], want["primary"]) and not PR.same_bits(now, ring)  # the block shows the update ...
    ring[:, :, fk:-fk, fk:-fk] = now[:, :, fk:-fk, fk:-fk]
    assert PR.same_bits(now, ring)  # ... and its faded margin is untouched
    us = P.ShareBlock.from_block_maps(bms[1], fk, ids[1], outmaps="US", postage_pad=pad)
    assert list(us.maps) == ["FIDELITY", "SIGMA"]
    with pytest.raises(ValueError, match="fade"):
        P.ShareBlock.from_block_maps(bms[1], fk + 1, ids[1], postage_pad=pad)


def test_refusals():
    import ctypes as C

    import torch

    from pyimcom_amd import _lib
    from pyimcom_amd import padshare as P

    a, b, c = H.pair_blocks("fk1")
    mine, theirs = share_block(a, c["n2"], c["postage_pad"], c["fk"]), share_block(b, c["n2"], c["postage_pad"], c["fk"])
    before = mine.to_arrays()
    with pytest.raises(ValueError, match="direction"):
        P.update(mine, theirs, "up")
    with pytest.raises(ValueError, match="itself"):
        P.update(mine, mine, "left")
    us_a, us_b, cu = H.pair_blocks("us")
    with pytest.raises(ValueError, match="maps"):
        P.update(mine, share_block(us_b, cu["n2"], cu["postage_pad"], cu["fk"]), "left")
    big = H.mosaic_blocks("in")[0][0]
    with pytest.raises(ValueError, match="shape"):
        P.update(mine, share_block(big, MOSAIC["n2"], MOSAIC["postage_pad"], MOSAIC["fk"]), "left")
    with pytest.raises(ValueError, match="fade_kernel"):
        P.update(mine, share_block(b, c["n2"], c["postage_pad"], c["fk"] + 1), "left")
    with pytest.raises(ValueError, match="n1P \\* n2"):
        share_block(a, c["n2"] + 1, c["postage_pad"], c["fk"])
    with pytest.raises(ValueError, match="float32"):
        P.ShareBlock.from_arrays(a["primary"].astype(np.float64), a["inweight"], a["idscas"], {}, c["n2"], c["postage_pad"], c["fk"])
    with pytest.raises(_lib.ImcomError, match="not a padding strip"):  # width < fk
        P.update(share_block(a, c["n2"], c["postage_pad"], 5), share_block(b, c["n2"], c["postage_pad"], 5), "left")
    with pytest.raises(_lib.ImcomError, match="not a padding strip"):  # 2 width > NsideP
        P.update(share_block(a, c["n2"], 3, 0), share_block(b, c["n2"], 3, 0), "left")
    # the entries themselves
    h, N = _lib.default_context().handle, c["n1P"] * c["n2"]
    pm, pu = mine.primary, theirs.primary
    layers = lambda d, w, fk, m=pm, u=pu: _lib.lib.imcom_padshare_layers(h, d, 1, N, w, fk, 4, _lib.ptr(m), N, N * N, _lib.ptr(u), N, N * N)  # noqa: E731
    for args in ((4, 4, 1), (-1, 4, 1), (0, 1, 2), (0, 9, 0)):
        assert layers(*args) == -1 and "not a padding strip" in _lib.lib.imcom_last_error().decode(), args
    assert layers(0, 4, 1, pm, pm) == -1 and "itself" in _lib.lib.imcom_last_error().decode()
    pairs = np.array([[0, 0]], dtype=np.int32)
    weights = lambda d, pad, n, p, u=theirs.inweight: _lib.lib.imcom_padshare_weights(h, d, 2, c["n1P"], pad, n, _lib.ptr(p), _lib.ptr(mine.inweight), 3, _lib.ptr(u), 4)  # noqa: E731
    assert weights(5, 1, 1, pairs) == -1 and weights(0, 3, 1, pairs) == -1 and "not a padding strip" in _lib.lib.imcom_last_error().decode()
    assert weights(0, 1, 1, np.array([[3, 0]], dtype=np.int32)) == -1 and "outside" in _lib.lib.imcom_last_error().decode()
    assert weights(0, 1, 2, np.array([[1, 0], [1, 2]], dtype=np.int32)) == -1 and "twice" in _lib.lib.imcom_last_error().decode()
    assert weights(0, 1, 1, pairs, mine.inweight) == -1 and "itself" in _lib.lib.imcom_last_error().decode()
    assert weights(0, 1, 0, None) == 0  # an empty table is a no-op
    row = (_lib.PadshareMap * 1)()
    row[0].mine, row[0].theirs, row[0].decode_coef, row[0].encode_coef = mine.maps["SIGMA"][0].data_ptr(), theirs.maps["SIGMA"][0].data_ptr(), -10000.0, -10000
    maps = lambda d, w, fk: _lib.lib.imcom_padshare_maps(h, d, 1, N, w, fk, 2, 1, C.cast(row, C.c_void_p))  # noqa: E731
    for args in ((4, 4, 1), (0, 1, 2), (0, 9, 0)):
        assert maps(*args) == -1 and "not a padding strip" in _lib.lib.imcom_last_error().decode(), args
    row[0].theirs = row[0].mine
    assert maps(0, 4, 1) == -1 and "itself" in _lib.lib.imcom_last_error().decode()
    row[0].theirs, row[0].decode_coef = theirs.maps["SIGMA"][0].data_ptr(), 0.0
    assert maps(0, 4, 1) == -1 and "descriptor" in _lib.lib.imcom_last_error().decode()
    assert _lib.lib.imcom_padshare_maps(h, 0, 1, N, 4, 1, 2, 0, None) == 0
    torch.cuda.synchronize()
    assert_block_equals(mine, {"primary": before["primary"], "inweight": before["inweight"], "maps": {k: list(v) for k, v in before["maps"].items()}})  # nothing was touched
