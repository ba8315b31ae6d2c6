"""CPU-side checks of the I24 codec (seam 14): the numpy restatement that the device tests compare with (tests/i24_reference.py) equals the
reference's fixtures with ==, the parameters are read and refused as the issue of the seam states, and csrc/i24_core.h -- the index maps,
the tile ranking and the tile scan that the kernels are made of -- agrees with plain loops under the sanitizers, as a host program."""

import json
import os
import subprocess

import numpy as np
import pytest

from tests import i24_reference as R
from tests.conftest import ROOT

G = np.load(os.path.join(ROOT, "tests", "golden", "i24.npz"))
NAMES = [str(n) for n in G["names"]]
FOREIGN = [str(n) for n in G["foreign_names"]]


def pars_of(name):
    return json.loads(str(G[f"{name}/pars"]))


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_reference(name):
    im, pars = G[f"{name}/in"], pars_of(name)
    a, tab = R.compress(im, "I24A", pars)
    b, tab_b = R.compress(im, "I24B", pars)
    assert a.dtype == np.int32 and b.dtype == np.uint8 and b.shape == ((int(pars.get("BITKEEP", 24)) + 7) // 8,) + im.shape
    assert np.array_equal(a, G[f"{name}/A"]) and np.array_equal(b, G[f"{name}/B"])
    for t in (tab, tab_b):
        assert np.array_equal(t[0], G[f"{name}/oy"]) and np.array_equal(t[1], G[f"{name}/ox"]) and np.array_equal(bits(t[2]), bits(G[f"{name}/ov"]))
    assert np.array_equal(bits(R.decompress(G[f"{name}/A"], "I24A", pars, tab)), bits(G[f"{name}/decA"]))
    assert np.array_equal(bits(R.decompress(G[f"{name}/B"], "I24B", pars, tab)), bits(G[f"{name}/decB"]))


@pytest.mark.parametrize("name", FOREIGN)
def test_restatement_decompresses_hand_made_inputs_as_the_reference(name):
    im = G[f"{name}/in"]
    assert np.array_equal(bits(R.decompress(im, "I24B" if im.dtype == np.uint8 else "I24A", pars_of(name))), bits(G[f"{name}/dec"]))


def test_restated_helpers_equal_the_reference():
    for k in range(4):
        cube = G[f"lsbf{k}/in"]
        assert np.array_equal(np.stack([R.stream_fwd(p) for p in cube]), G[f"lsbf{k}/fwd"])
        assert np.array_equal(np.stack([R.stream_rev(p) for p in cube]), G[f"lsbf{k}/rev"])
    for k in range(3):
        q, B = G[f"int{k}/in"], int(G[f"int{k}/bitkeep"])
        assert np.array_equal(R.ints_fwd(q, B, 0, True), G[f"int{k}/diff_fwd"]) and np.array_equal(R.ints_rev(q, B, 0, True), G[f"int{k}/diff_rev"])
        assert np.array_equal(R.ints_fwd(q, B, -1, False), G[f"int{k}/small_fwd"]) and np.array_equal(R.ints_rev(q, B, -1, False), G[f"int{k}/small_rev"])


def test_the_fixture_holds_the_edges_it_is_there_for():
    n_over = {n: len(G[f"{n}/oy"]) for n in NAMES}
    assert min(n_over.values()) == 0 and n_over["edge5x13_bNone"] >= 6
    im, ov = G["edge33x65_b17/in"], G["edge33x65_b17/ov"]
    assert np.isnan(im).sum() == 1 and not np.isnan(ov).any() and np.isinf(ov).sum() >= 2  # NaN: no entry; both infinities: entries
    lo, hi = np.float32(0.1), np.float32(0.7)
    assert lo in im and hi in im and lo not in ov and hi not in ov
    assert np.nextafter(lo, np.float32(-1)) in ov and np.nextafter(hi, np.float32(1)) in ov
    assert pars_of("string_false")["DIFF"] == "False" and not np.array_equal(G["string_false/A"], R.quantise(G["string_false/in"], -0.5, 1.5, 16))
    assert (G["s3x5_b20_r1/B"].shape, G["s1x1_b7_r1/B"].shape) == ((3, 3, 5), (1, 1, 1))


def test_parameters_are_read_as_the_reference_reads_them():
    from pyimcom_amd import i24

    p = i24.parse_pars({"VMIN": "0.1", "VMAX": 7})
    assert (p.vmin, p.vmax, p.alpha, p.softbias, p.bitkeep, p.diff, p.reorder) == (0.1, 7.0, 1.0, 0, 24, 0, 1)
    p = i24.parse_pars({"VMIN": 0, "VMAX": 1, "DIFF": "False", "REORDER": "False", "BITKEEP": "20", "SOFTBIAS": -1.0, "ALPHA": "1.0"})
    assert (p.diff, p.reorder, p.bitkeep, p.softbias, p.alpha) == (1, 1, 20, -1, 1.0)  # the string "False" is true, as in the reference
    assert i24.parse_pars({"VMIN": 0, "VMAX": 1, "DIFF": 0, "REORDER": False, "SOFTBIAS": -10**30}).softbias < -1
    for bad in (24, 25, 0, -3):
        with pytest.raises(ValueError, match="Can't keep"):
            i24.parse_pars({"VMIN": 0, "VMAX": 1, "BITKEEP": bad})
        with pytest.raises(ValueError, match="Can't keep"):
            R.parse({"VMIN": 0, "VMAX": 1, "BITKEEP": bad})
    with pytest.raises(KeyError):
        i24.parse_pars({"VMAX": 1})


def test_refusals():
    from pyimcom_amd import _lib, i24

    def status(pars, ny=4, nx=4, match=None):
        with pytest.raises(_lib.ImcomError, match=match) as e:
            i24.check_pars([{"VMIN": 0.0, "VMAX": 1.0}, pars], ny, nx)
        return e.value.status

    i24.check_pars([{"VMIN": 0.0, "VMAX": 1.0, "ALPHA": 1.0, "SOFTBIAS": 2**24 - 1}, {"VMIN": -1, "VMAX": 1, "SOFTBIAS": -7, "BITKEEP": 1}], 3, 5)
    assert status({"VMIN": 0.0, "VMAX": 1.0, "ALPHA": 0.5}, match="ALPHA") == -4  # IMCOM_ERR_UNSUPPORTED, and the message says why
    assert status({"VMIN": 0.0, "VMAX": 1.0, "ALPHA": float("nan")}) == -4
    assert status({"VMIN": 1.0, "VMAX": 1.0}, match="VMAX") == -1
    assert status({"VMIN": 1.0, "VMAX": 0.0}) == -1
    for v in (float("inf"), float("-inf"), float("nan")):
        assert status({"VMIN": 0.0, "VMAX": v}) == -1 and status({"VMIN": v, "VMAX": 1.0}) == -1
    assert status({"VMIN": 0.0, "VMAX": 1.0, "SOFTBIAS": 2**24}, match="SOFTBIAS") == -1
    assert status({"VMIN": 0.0, "VMAX": 1.0, "SOFTBIAS": 2**70}) == -1
    assert status({"VMIN": 0.0, "VMAX": 1.0}, ny=65536, nx=32768, match="pixels") == -1  # ny nx = 2^31
    i24.check_pars([{"VMIN": 0.0, "VMAX": 1.0}], 65536, 32767)
    # a cube whose first axis is not (BITKEEP + 7) // 8: refused before anything is sent to a device
    for planes, bk in ((3, 16), (2, 17), (1, 9), (2, None)):
        pars = {"VMIN": 0.0, "VMAX": 1.0}
        if bk:
            pars["BITKEEP"] = bk
        with pytest.raises(_lib.ImcomError, match="byte planes") as e:
            i24.i24decompress(np.zeros((planes, 4, 4), dtype=np.uint8), "I24B", pars)
        assert e.value.status == -1
    # an unrecognised scheme hands the input back
    im = np.zeros((2, 2), dtype=np.float32)
    assert i24.i24compress(im, "I16", {})[0] is im and i24.i24compress(im, "I16", {})[1] is None and i24.i24decompress(im, "none", {}) is im
    with pytest.raises(TypeError):
        i24.i24compress(np.zeros((2, 2), dtype=np.float64), "I24B", {"VMIN": 0, "VMAX": 1})
    with pytest.raises(TypeError):
        i24.i24decompress(np.zeros((2, 2), dtype=np.uint8), "I24B", {"VMIN": 0, "VMAX": 1})


def test_sizes_give_the_tile_constants_of_the_header():
    from pyimcom_amd import i24

    tile, chunk = i24.tile_constants()
    assert tile >= 64 and tile % 64 == 0 and chunk >= 1  # (whole waves; the device tests aim at multiples of these)
    recs = i24._records([{"VMIN": 0, "VMAX": 1, "BITKEEP": 9}, {"VMIN": 0, "VMAX": 1, "BITKEEP": 17}])
    sz = i24._sizes(recs, 100, 41, "I24B")
    tiles = -(-4100 // tile)
    assert sz[3] == 3 * 4100 and sz[4] == tiles and sz[5:7] == [tile, chunk] and sz[0] == (2 * tiles + 2) * 4 and sz[1] >= 2 * 4100 * 4 and sz[2] >= sz[1]
    assert i24._sizes(recs, 100, 41, "I24A")[3] == 4 * 4100


def test_overflow_table_object():
    from pyimcom_amd import i24

    t = i24.OverflowTable(np.array([1, 2], dtype=np.int32), np.array([3, 4], dtype=np.int32), np.array([0.5, 1.5], dtype=np.float32))
    assert len(t) == 2 and [c.dtype for c in t.columns()] == [np.int32, np.int32, np.float32] and t.data["x"][1] == 4


def test_native_core_against_plain_loops_under_sanitizers(tmp_path):
    exe = tmp_path / "i24_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "pyimcom_amd", "csrc"), os.path.join(ROOT, "tests", "native", "i24_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.strip().splitlines()]
    assert [r[0] for r in rows] == ["stream", "rank", "scan", "ints"]
    assert all(int(r[1]) > 1000 and int(r[2]) == 0 for r in rows), rows
