"""numpy's Poisson draws without a device: the Python restatement (tests/poisson_reference.py) against ``Generator.poisson``, the
host-compilable core of the kernels with its window tables and recovery (csrc/poisson_core.h) as a stand-alone program under the address
and undefined-behaviour sanitizers (tests/native/poisson_check.cpp), the parsing of the layer name, the layer formula, and the golden of
the reference's own statements (tests/golden/nstar.npz, made by tests/golden/make_golden_nstar.py)."""

import os
import subprocess

import numpy as np
import pytest

from tests import poisson_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [0, 12345, 1000000 * (18 * 3 + 7) + 4242]


def rate_cases():
    """name -> rates: what the restatement must cover."""
    rng = np.random.default_rng(2024)
    mix = np.concatenate([np.zeros(300), rng.uniform(0.0, 10.0, 3000), rng.uniform(10.0, 3010.0, 5000), np.full(200, 10.0), np.full(100, 2.0e5),
                          np.full(2000, 86.0), np.full(200, np.nextafter(10.0, 0.0))])
    rng.shuffle(mix)
    zeros = np.full(4000, 86.0)
    zeros[100:164] = 0.0  # a run
    zeros[1000] = zeros[1002] = zeros[3999] = 0.0  # alone, and the last draw
    zeros[2000:2040:2] = 0.0
    return {
        "86": np.full(20000, 86.0), "10": np.full(5000, 10.0), "below10": np.full(5000, np.nextafter(10.0, 0.0)), "0.5": np.full(5000, 0.5),
        "3": np.full(5000, 3.0), "9.9": np.full(5000, 9.9), "zeros": zeros, "2e5": np.full(5000, 2.0e5), "mix": mix,
    }


CASES = rate_cases()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_numpy_draws_and_state(name, seed):
    lam = CASES[name]
    r = pr.poisson_from_raw(pr.raw_for(seed, lam), lam)
    bg = np.random.PCG64(seed)
    want = np.random.Generator(bg).poisson(lam=lam)
    assert want.dtype == np.int64 and r["values"].tobytes() == want.tobytes()
    ref = np.random.PCG64(seed)
    ref.advance(r["consumed"])
    assert ref.state == bg.state
    expect = {"86": {pr.PTRS}, "10": {pr.PTRS}, "below10": {pr.MULT}, "0.5": {pr.MULT}, "3": {pr.MULT}, "9.9": {pr.MULT}, "zeros": {pr.ZERO, pr.PTRS},
              "2e5": {pr.PTRS}, "mix": {pr.ZERO, pr.MULT, pr.PTRS}}[name]
    assert set(r["branch"].tolist()) == expect
    assert np.all(r["adv"][r["branch"] == pr.ZERO] == 0) and np.all(r["adv"][r["branch"] == pr.MULT] == r["values"][r["branch"] == pr.MULT] + 1)
    if name == "86":  # every outcome of an attempt occurs, and the consumption is the measured 2.36 outputs a draw
        assert {o for os_ in r["outcomes"] for o in os_} == {pr.FAST, pr.QUICK_REJECT, pr.SLOW_ACCEPT, pr.SLOW_REJECT}
        assert abs(r["consumed"] / lam.size - 2.356) < 0.03


def test_numpys_value_errors():
    for bad in (-1.0, np.nan, 1.0e19, -np.inf):
        lam = np.array([86.0, bad])
        assert not (lam[1] >= 0.0 and lam[1] <= pr.LAM_MAX)
        with pytest.raises(ValueError):
            np.random.default_rng(0).poisson(lam=lam)
    np.random.default_rng(0).poisson(lam=np.array([0.0, pr.LAM_MAX]))  # the largest rate numpy takes


def _write_case(path, seed, lam):
    raw = pr.raw_for(seed, lam)
    r = pr.poisson_from_raw(raw, lam)
    assert not r["flags"].any()
    with open(path, "wb") as f:
        f.write(np.array([len(raw), lam.size, r["consumed"]], dtype=np.int64).tobytes())
        f.write(np.asarray(raw, dtype=np.uint64).tobytes())
        f.write(np.asarray(lam, dtype=np.float64).tobytes())
        f.write(r["values"].astype(np.int64).tobytes())
        f.write(r["adv"].astype(np.int64).tobytes())
    return r


def test_native_core_equals_the_restatement_under_sanitizers(tmp_path):
    """poi_draw one draw after another, and the window tables with their recovery for S in {4, 64}, W in {2, 8, 64}, T in {4, 16}, with the
    production guard band and with none, on: constant 86, the mix of all branches, a frame with runs of zero rates, rates below 10 (whose
    excess grows by lam a draw), and no draws at all.  The narrow windows must have been left (the recovery ran), the widest not always."""
    exe = tmp_path / "poisson_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "pyimcom_amd", "csrc"), os.path.join(ROOT, "tests", "native", "poisson_check.cpp"), "-o", str(exe)])
    files = []
    for name, lam, seed in (("c86", CASES["86"][:3000], 7), ("mix", CASES["mix"][:3000], 8), ("zeros", CASES["zeros"][:1100], 9),
                            ("low", CASES["9.9"][:500], 10), ("empty", np.zeros(0), 11)):
        _write_case(tmp_path / (name + ".bin"), seed, lam)
        files.append(str(tmp_path / (name + ".bin")))
    out = subprocess.run([str(exe)] + files, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.strip().splitlines()]
    assert [r[1] for r in rows] == ["36"] * 5
    assert int(rows[0][2]) > 0 and int(rows[1][2]) > 0 and int(rows[4][2]) == 0
    assert rows[0][3:] == ["0", "0", "3000"] and all(int(v) > 0 for v in rows[1][3:]) and rows[4][3:] == ["0", "0", "0"]


def test_window_model_of_the_restatement():
    """The restated window scheme: with W = 2 a path at 86 leaves the window at its first refused attempt; with a window that covers every
    excess the path can reach it never does; a wide guard band shows undecided nodes."""
    lam = np.full(64, 86.0)
    raw = pr.raw_for(3, lam)
    path = pr.poisson_from_raw(raw, lam)
    assert path["consumed"] > 2 * lam.size
    assert any(w["leaves"] for w in pr.windows(raw, lam, 16, 2))
    assert not any(w["leaves"] for w in pr.windows(raw, lam, 16, 64))
    wide = pr.windows(raw, lam, 64, 8, guard=1.0e-3)
    assert wide[0]["on_path"] | (wide[0]["off_path"] > 0)
    assert pr.drift256(86.0) == 91 and pr.drift256(0.0) == 0 and pr.drift256(3.0) == 768 and pr.min_adv(0.0) == 0 and pr.min_adv(9.9) == 1


def test_parse_nstar_reads_the_references_strings():
    from pyimcom_amd.inject import parse_nstar

    assert parse_nstar("nstar14,2e5,86,3") == (14, 2.0e5, 86.0, 3)
    assert parse_nstar("NSTAR13,40.0,3.5,1") == (13, 40.0, 3.5, 1)
    assert parse_nstar("cstar14") is None and parse_nstar("whitenoise3") is None and parse_nstar("nstar,1,2,3") is None
    res, tot_int, bg, q = parse_nstar("nstar14,2e5,86,3")
    assert isinstance(res, int) and isinstance(tot_int, float) and isinstance(bg, float) and isinstance(q, int)


def _layer_numpy(brightness, tot_int, bg, q, idsca):
    """layer.py:1364-1387 written out with numpy."""
    rng = np.random.default_rng(1000000 * (18 * q + idsca[1]) + idsca[0])
    lam = brightness * tot_int + bg
    _lam = np.clip(lam, 0, None)
    return (rng.poisson(lam=_lam) - _lam + lam - bg).astype(np.float32), lam, _lam


def test_layer_formula_where_the_brightness_is_negative():
    """Where lam < 0 the draw is of rate 0 and the layer is ((0 - 0) + lam) - bg = brightness * tot_int up to rounding: no noise; the
    restatement's draws of the clipped rates give the same layer as numpy's."""
    rng = np.random.default_rng(5)
    brightness = rng.normal(0.0, 1.0e-3, (32, 32))
    tot_int, bg, q, idsca = 2.0e5, 86.0, 3, (1234, 5)
    layer, lam, _lam = _layer_numpy(brightness, tot_int, bg, q, idsca)
    assert (lam < 0).any() and (_lam != lam).any()
    seed = 1000000 * (18 * q + idsca[1]) + idsca[0]
    r = pr.poisson_from_raw(pr.raw_for(seed, _lam), _lam)
    mine = (((r["values"].reshape(lam.shape).astype(np.float64) - _lam) + lam) - bg).astype(np.float32)
    assert mine.tobytes() == layer.tobytes()
    neg = lam < 0
    assert np.all(r["values"].reshape(lam.shape)[neg] == 0) and np.array_equal(layer[neg], ((lam - bg)[neg]).astype(np.float32))


def test_golden_of_the_references_statements():
    """tests/golden/nstar.npz holds what the reference's statements gave; numpy's statements written out here and the restatement give the
    same, and the second setting reaches every branch."""
    from pyimcom_amd.inject import parse_nstar

    g = np.load(os.path.join(ROOT, "tests", "golden", "nstar.npz"))
    branches = set()
    for k, string in enumerate(g["strings"].tolist()):
        res, tot_int, bg, q = parse_nstar(string)
        idsca = tuple(int(v) for v in g["idsca"][k])
        brightness = g[f"brightness{k}"]
        assert brightness.shape == (64, 64) and (brightness < 0).any()
        layer, lam, _lam = _layer_numpy(brightness, tot_int, bg, q, idsca)
        assert layer.tobytes() == g[f"layer{k}"].tobytes()
        seed = 1000000 * (18 * q + idsca[1]) + idsca[0]
        r = pr.poisson_from_raw(pr.raw_for(seed, _lam), _lam)
        assert ((((r["values"].reshape(lam.shape) - _lam) + lam) - bg).astype(np.float32)).tobytes() == g[f"layer{k}"].tobytes()
        branches |= set(r["branch"].tolist())
    assert branches == {pr.ZERO, pr.MULT, pr.PTRS}
