"""CPU-side checks of the shared padding stamps (seam 20): the numpy restatement (tests/padshare_reference.py) against
tests/golden/padshare.npz, which holds what the reference's own statements gave; the host decisions of pyimcom_amd.padshare (the decode
coefficient, the floor rule under the installed numpy, the exposure pairing); csrc/padshare_core.h as a host program under the sanitizers;
the null-context refusal of the new entries.  Everything is compared bit for bit."""

import json
import os
import subprocess

import numpy as np
import pytest

from tests import padshare_reference as PR
from tests.conftest import ROOT

G = np.load(os.path.join(ROOT, "tests", "golden", "padshare.npz"))
META = json.loads(str(G["meta"]))
MOSAIC = META["mosaic"]
UNITS = {k: tuple(v) for k, v in META["units"].items()}
PAIRS = sorted(META["pairs"])
ENTRIES = ["imcom_padshare_layers", "imcom_padshare_weights", "imcom_padshare_maps"]
# zero_floor=None of the restatement is what the generator recorded only under the same rule, which depends on numpy's major version
SAME_NUMPY_RULE = (int(np.__version__.split(".")[0]) >= 2) == (int(META["numpy"].split(".")[0]) >= 2)
AUTO = None


def mosaic_blocks(which):
    return [[PR.fixture_block(G, f"mosaic_{which}_{iby}_{ibx}", UNITS, MOSAIC["idscas"][f"{iby},{ibx}"]) for ibx in range(3)] for iby in range(3)]


def pair_blocks(name):
    c = META["pairs"][name]
    units = {k: tuple(v) for k, v in c["maps"].items()}
    return PR.fixture_block(G, f"pair_{name}_mine", units, c["mine_idscas"]), PR.fixture_block(G, f"pair_{name}_theirs", units, c["theirs_idscas"]), c


def pair_expected(name, k, mine, c):
    """``mine`` after call k of the pair case: the input with my strip replaced by the recorded one; and the recorded sums."""
    direction, _ = c["calls"][k]
    N, n1P = c["n1P"] * c["n2"], c["n1P"]
    my, _ = PR.strips(direction, N, c["postage_pad"] * c["n2"], c["fk"])
    wmy, _ = PR.strips(direction, n1P, c["postage_pad"], 0)
    want = PR.copy_block(mine)
    for key, s, arr in [("primary", my, want["primary"]), ("inweight", wmy, want["inweight"])] + [(n, my, want["maps"][n][0]) for n in want["maps"]]:
        view = PR.strip_of(arr, direction, s)
        view[...] = G[f"pair_{name}_out_{key}"][k].reshape(view.shape)
    sums = {n: G[f"pair_{name}_out_sums_{n}"][k].reshape(PR.strip_of(want["maps"][n][0], direction, my).shape) for n in want["maps"]}
    return want, sums


def blocks_equal(a, b):
    return (PR.same_bits(a["primary"], b["primary"]) and PR.same_bits(a["inweight"], b["inweight"]) and list(a["maps"]) == list(b["maps"])
            and all(PR.same_bits(a["maps"][n][0], b["maps"][n][0]) for n in a["maps"]))


def test_the_fixture_was_written_under_this_numpys_floor_rule():
    assert SAME_NUMPY_RULE, f"tests/golden/padshare.npz was written beside numpy {META['numpy']}: regenerate it with the numpy the reference runs beside"


def test_the_fixture_holds_the_cases_the_issue_lists():
    m = MOSAIC
    assert (m["n2"], m["postage_pad"], m["n1P"], m["fk"], m["nblock"], m["n_out"], m["nlayer"]) == (4, 2, 8, 2, 3, 2, 3) and list(UNITS) == list(PR.MAPS)
    assert G["mosaic_in_1_1_primary"].shape == (2, 3, 32, 32) and G["mosaic_in_1_1_SIGMA"].dtype == np.dtype(">i2") and G["mosaic_in_1_1_EFFCOVER"].dtype == np.uint16
    assert [s for s in m["order"] if s[0] == "update" and s[1] == [1, 1]] == [["update", [1, 1], [1, 0], "left", False], ["update", [1, 1], [1, 2], "right", True],
                                                                            ["update", [1, 1], [0, 1], "bottom", False], ["update", [1, 1], [2, 1], "top", True]]
    for name, (letter, coef, dtype, unit, comment) in PR.MAPS.items():  # runs of the floor code and of the saturated code, and codes between
        lo, hi = PR.code_range(dtype)
        codes = G[f"mosaic_in_1_1_{name}"]
        assert (codes == lo).sum() > 100 and (codes == hi).sum() > 100 and ((codes > lo) & (codes < hi)).sum() > 100
    p = G["mosaic_in_1_0_primary"]
    assert (p == 0).any() and (p < 0).any() and np.signbit(p[0, 0, 12, 17]) and p[0, 0, 12, 17] == 0 and np.isinf(G["mosaic_in_1_1_primary"][1, 0, 13, 2])
    out, left = G["mosaic_out_1_1_primary"], G["mosaic_out_1_0_primary"]
    assert np.signbit(left[0, 0, 14, 25]) and left[0, 0, 14, 25] == 0 and left[1, 2, 15, 26] == -np.inf  # -0.0 + -0.0 of the add call, and -inf passed on
    assert out[0, 0, 12, 1] == 0 and not np.signbit(out[0, 0, 12, 1]) and np.isnan(out[1, 0, 13, 2])  # -0.0 arrived as +0.0, inf * False as NaN
    ids = {k: [tuple(p) for p in v] for k, v in m["idscas"].items()}
    assert len({len(v) for v in ids.values()}) > 2 and not set(ids["1,0"]) & set(ids["2,0"]) and len(ids["0,1"]) != len(set(ids["0,1"]))
    assert {(c["fk"], c["postage_pad"], c["n2"]) for c in META["pairs"].values()} == {(0, 1, 4), (1, 1, 4), (2, 1, 4)}
    assert list(META["pairs"]["us"]["maps"]) == ["FIDELITY", "SIGMA"] and META["pairs"]["legacy"]["maps"] == {"FIDELITY": ["0.2mB", "-5000*log10(U/C)"]}
    assert all(len(c["calls"]) == 8 and len({tuple(x) for x in c["calls"]}) == 8 for c in META["pairs"].values())
    assert META["encode"]["add_worst_share"] <= META["cap"] == 0.01 and META["encode"]["add_strips"] > 100
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "padshare.npz")) < 495_294  # (the largest fixture before it)


def test_restatement_runs_the_loop_as_the_reference_did():
    blocks = mosaic_blocks("in")
    assert [list(s[:1]) + [list(v) if isinstance(v, tuple) else v for v in s[1:]] for s in PR.share_order(3)] == MOSAIC["order"]
    recorded = {}
    for step in PR.share_order(3):
        if step[0] == "update":
            (ay, ax), (by, bx) = step[1], step[2]
            sums = PR.update(blocks[ay][ax], blocks[by][bx], step[3], step[4], MOSAIC["n2"], MOSAIC["postage_pad"], MOSAIC["fk"], AUTO)
            if (ay, ax) == (1, 1):
                recorded[step[3]] = sums
    want = mosaic_blocks("out")
    for iby in range(3):
        for ibx in range(3):
            assert blocks_equal(blocks[iby][ibx], want[iby][ibx]), (iby, ibx)
    assert sorted(recorded) == sorted(PR.DIRECTIONS)
    for direction, sums in recorded.items():
        for name in sums:
            assert PR.same_bits(sums[name], G[f"mosaic_sums_{direction}_{name}"]), (direction, name)


@pytest.mark.parametrize("name", PAIRS)
def test_restatement_of_the_pair_cases(name):
    mine, theirs, c = pair_blocks(name)
    for k, (direction, add_mode) in enumerate(c["calls"]):
        got, ur = PR.copy_block(mine), PR.copy_block(theirs)
        sums = PR.update(got, ur, direction, add_mode, c["n2"], c["postage_pad"], c["fk"], AUTO)
        want, want_sums = pair_expected(name, k, mine, c)
        assert blocks_equal(got, want) and blocks_equal(ur, theirs), (direction, add_mode)
        assert all(PR.same_bits(sums[n], want_sums[n]) for n in sums), (direction, add_mode)
        if not add_mode:  # decode then encode returns the code: my strip holds the neighbour's codes
            my, urs = PR.strips(direction, c["n1P"] * c["n2"], c["postage_pad"] * c["n2"], c["fk"])
            assert all(np.array_equal(PR.strip_of(got["maps"][n][0], direction, my), PR.strip_of(theirs["maps"][n][0], direction, urs)) for n in sums)


def codes_within_the_allowance(got, want, direction=None, strip=None):
    """The condition of tests/test_gpu_block.py for codes that the two log10 may encode differently: never more than one count apart, and
    different for at most 1 % of the pixels (of my strip, or of the whole map)."""
    a, b = (np.asarray(v).astype(np.int64) for v in (got, want))
    if strip is not None:
        outside = np.ones(a.shape[-1], dtype=bool)
        outside[strip] = False
        if not np.array_equal(PR.strip_of(a, direction, outside), PR.strip_of(b, direction, outside)):
            return False
        a, b = PR.strip_of(a, direction, strip), PR.strip_of(b, direction, strip)
    d = np.abs(a - b)
    return bool(d.max() <= 1 and np.mean(d != 0) <= META["cap"])


def device_formula_mosaic():
    """The mosaic case by the restatement with the device's encode (log10 correctly rounded to float32): what the kernels must give exactly."""
    blocks = mosaic_blocks("in")
    sums = []
    for step in PR.share_order(3):
        if step[0] == "update":
            (ay, ax), (by, bx) = step[1], step[2]
            sums.append(PR.update(blocks[ay][ax], blocks[by][bx], step[3], step[4], MOSAIC["n2"], MOSAIC["postage_pad"], MOSAIC["fk"], AUTO, encode=PR.compress_device))
    return blocks, sums


def test_the_devices_encode_stays_within_the_allowance_over_the_whole_loop():
    """A code that the device's log10 encodes one count apart is read again by later calls of the loop; the maps after the full loop still
    lie within one count of the reference's for at most 1 % of each map's pixels, and everything that is no code is unaffected."""
    blocks, _ = device_formula_mosaic()
    want = mosaic_blocks("out")
    for iby in range(3):
        for ibx in range(3):
            got, ref = blocks[iby][ibx], want[iby][ibx]
            assert PR.same_bits(got["primary"], ref["primary"]) and PR.same_bits(got["inweight"], ref["inweight"])
            assert all(codes_within_the_allowance(got["maps"][n][0], ref["maps"][n][0]) for n in ref["maps"]), (iby, ibx)


def test_decode_then_encode_returns_every_code():
    """What makes the codes of a replace call an equality: for all 65536 codes of the five maps, under either floor rule and either log10."""
    for name, (letter, coef, dtype, unit, comment) in PR.MAPS.items():
        lo, hi = PR.code_range(dtype)
        codes = np.arange(lo, hi + 1).astype(dtype)
        for zero_floor in (True, False):
            values = PR.decode(codes, unit, comment, zero_floor)
            assert np.array_equal(PR.compress(values, coef, dtype), codes) and np.array_equal(PR.compress_device(values, coef, dtype), codes), (name, zero_floor)


def test_the_floor_rule_is_the_installed_numpys():
    from pyimcom_amd import padshare as P

    for name, (letter, coef, dtype, unit, comment) in PR.MAPS.items():
        unsigned = np.dtype(dtype) == np.uint16
        lo, hi = PR.code_range(dtype)
        a_zero = lo if coef > 0 else hi
        assert P.decode_coefficient(unit, comment) == 1.0 / PR.unit_to_bels(unit, comment) and repr(P.decode_coefficient(unit, comment)) == META["decode_coef"][name]
        assert P.floor_code(unit, comment, unsigned, True) == a_zero and P.floor_code(unit, comment, unsigned, False) is None
        # the reference's own statements (analysis.py:379, 387) on the one code, with the installed numpy
        data = np.power(10.0, np.array([a_zero], dtype=dtype) / (1.0 / PR.unit_to_bels(unit, comment))).astype(np.float32)
        zeroes = bool((data == np.power(10.0, a_zero / (1.0 / PR.unit_to_bels(unit, comment))))[0])
        assert P.floor_code(unit, comment, unsigned) == (a_zero if zeroes else None)
        if int(np.__version__.split(".")[0]) >= 2:  # float64 comparison: true only where the power is exactly a float32
            assert zeroes == (name == "EFFCOVER")
        else:  # the scalar is demoted: every floor code is zeroed
            assert zeroes
        if SAME_NUMPY_RULE:
            assert META["floor_rule"][name] == [zeroes, not zeroes]
    assert P.decode_coefficient("0.2mB", "-5000*log10(U/C)") == -5000.0 and P.decode_coefficient("0.2mB", "5000*log10(x)") == 5000.0  # the legacy sign fix
    assert np.isnan(P.unit_to_bels("unknown", "x"))


def test_exposures_are_paired_by_first_occurrence():
    from pyimcom_amd import padshare as P

    my, ur = [(1, 1), (2, 2), (3, 3)], [(3, 3), (4, 4), (1, 1), (3, 3)]
    assert P.idsca_pairs(my, ur).tolist() == [[0, 2], [2, 0]] and P.idsca_pairs(ur, my).tolist() == [[0, 2], [2, 0]]
    assert P.idsca_pairs([(1, 1)], [(2, 2)]).shape == (0, 2) and P.idsca_pairs([(1, 1)], [(2, 2)]).dtype == np.int32
    for c in META["pairs"].values():
        assert P.idsca_pairs(c["mine_idscas"], c["theirs_idscas"]).tolist() == c["pairs"]
    ids = MOSAIC["idscas"]
    for a in ids:
        for b in ids:
            assert P.idsca_pairs(ids[a], ids[b]).tolist() == [list(p) for p in PR.pairs(ids[a], ids[b])]
    assert P.idsca_pairs(ids["1,0"], ids["2,0"]).shape == (0, 2)
    assert P.idsca_pairs(ids["0,1"], ids["0,0"]).tolist() == [[0, 1], [1, 0]]  # the repeated (11, 3) of (0, 1) counts once, at its first place


# ---- the core as a host program ---------------------------------------------------------------------------------------------------------

def _f64_bits(v):
    return int(np.array([v], dtype=np.float64).view(np.int64)[0])


def _words(a):
    a = np.ascontiguousarray(np.asarray(a).astype(np.asarray(a).dtype.newbyteorder("=")))
    if a.dtype.kind == "f":
        return a.view(np.uint32).astype(np.int64).ravel()
    return a.view(np.uint16).astype(np.int64).ravel()


def _jobs_of_call(jobs, mine, theirs, direction, add_mode, n2, pad, fk, counts):
    """One update as planes: the restatement with the device's encode gives the expected codes (the recorded ones for a replace call)."""
    want, ur = PR.copy_block(mine), PR.copy_block(theirs)
    sums = PR.update(want, ur, direction, add_mode, n2, pad, fk, AUTO, encode=PR.compress_device)
    d, N, n1P = PR.DIRECTIONS.index(direction), mine["primary"].shape[-1], mine["inweight"].shape[-1]
    for o in range(mine["primary"].shape[0]):
        for l in range(mine["primary"].shape[1]):
            jobs.append(np.concatenate(([0, d, int(add_mode), N, pad * n2, fk], _words(mine["primary"][o, l]), _words(theirs["primary"][o, l]), _words(want["primary"][o, l]))))
            counts["layers"] += N * N
        for i, j in PR.pairs(mine["idscas"], theirs["idscas"]):
            jobs.append(np.concatenate(([2, d, n1P, pad], _words(mine["inweight"][o, i]), _words(theirs["inweight"][o, j]), _words(want["inweight"][o, i]))))
            counts["weights"] += n1P * n1P
        for name, (codes, unit, comment) in mine["maps"].items():
            coef = 1.0 / PR.unit_to_bels(unit, comment)
            lo, hi = PR.code_range(codes.dtype)
            a_zero = lo if coef > 0 else hi
            zeroed = bool(PR.decode(np.array([a_zero]).astype(codes.dtype), unit, comment, AUTO)[0] == 0.0)
            jobs.append(np.concatenate(([1, d, int(add_mode), N, pad * n2, fk, _f64_bits(coef), a_zero if zeroed else 1 << 20, int(comment.partition("*")[0]), int(lo == 0)],
                                        _words(codes[o]), _words(theirs["maps"][name][0][o]), _words(want["maps"][name][0][o]), _words(sums[name][o]))))
            counts["maps"] += N * N
            counts["sums"] += sums[name][o].size
    return want


def _jobs_file(path):
    jobs, counts = [], {"layers": 0, "maps": 0, "sums": 0, "weights": 0}
    for name in PAIRS:
        mine, theirs, c = pair_blocks(name)
        for k, (direction, add_mode) in enumerate(c["calls"]):
            want = _jobs_of_call(jobs, mine, theirs, direction, add_mode, c["n2"], c["postage_pad"], c["fk"], counts)
            recorded, _ = pair_expected(name, k, mine, c)
            assert PR.same_bits(want["primary"], recorded["primary"]) and PR.same_bits(want["inweight"], recorded["inweight"])
            if not add_mode:  # (an add call's codes may differ by the one count that the two log10 allow; its sums may not)
                assert all(PR.same_bits(want["maps"][n][0], recorded["maps"][n][0]) for n in want["maps"])
    blocks = mosaic_blocks("in")  # the loop's first two calls at the mosaic's shape (n_out = 2, three layers, fk = 2)
    _jobs_of_call(jobs, blocks[0][0], blocks[0][1], "right", True, MOSAIC["n2"], MOSAIC["postage_pad"], MOSAIC["fk"], counts)
    _jobs_of_call(jobs, blocks[1][1], blocks[0][1], "bottom", False, MOSAIC["n2"], MOSAIC["postage_pad"], MOSAIC["fk"], counts)
    np.concatenate([np.array([len(jobs)], dtype=np.int64)] + [np.asarray(j, dtype=np.int64) for j in jobs]).tofile(path)
    return counts


def test_native_core_against_the_fixture_under_sanitizers(tmp_path):
    exe, jobs = tmp_path / "padshare_check", tmp_path / "jobs.bin"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "pyimcom_amd", "csrc"), os.path.join(ROOT, "tests", "native", "padshare_check.cpp"), "-o", str(exe)])
    counts = _jobs_file(str(jobs))
    out = subprocess.run([str(exe), str(jobs)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.strip().splitlines()]
    assert [r[0] for r in rows] == ["layers", "maps", "sums", "weights"]
    assert all(int(r[1]) == counts[r[0]] and int(r[1]) > 0 and int(r[2]) == 0 for r in rows), (rows, counts)


# ---- the boundary -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ENTRIES)
def test_null_context_is_refused_before_anything_else(name):
    import ctypes as C

    from pyimcom_amd import _lib

    def null(t):
        if t in (C.c_double, C.c_float):
            return 0.0
        return 0 if isinstance(t, type) and issubclass(t, C._SimpleCData) and t._type_ in "bBhHiIlLqQ" else None

    assert getattr(_lib.lib, name)(*[null(t) for t in _lib.SIGNATURES[name]]) == -1
    assert "null context" in _lib.lib.imcom_last_error().decode()


def test_descriptor_matches_the_header():
    """The ctypes mirror of imcom_padshare_map has the C struct's layout (48 bytes, the double at 16)."""
    import ctypes as C

    from pyimcom_amd import _lib

    assert C.sizeof(_lib.PadshareMap) == 48 and _lib.PadshareMap.decode_coef.offset == 16 and _lib.PadshareMap.floor_code.offset == 32
    txt = open(os.path.join(ROOT, "include", "imcom_hip.h")).read()
    assert "#define IMCOM_PADSHARE_NO_FLOOR (1 << 20)" in txt and _lib.PADSHARE_NO_FLOOR == 1 << 20
