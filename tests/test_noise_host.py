"""numpy's normal draws without a device: the integer restatement (tests/noise_reference.py) against ``Generator.standard_normal``, the
committed tables (csrc/ziggurat_tables.h) against the installed numpy through crafted PCG64 states, and the host-compilable core of the
kernels (csrc/ziggurat_core.h) as a stand-alone program under the address and undefined-behaviour sanitizers
(tests/native/ziggurat_check.cpp)."""

import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import noise_reference as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABS = nr.tables()


def _raw_and_draws(seed, count):
    """(raw outputs with room to spare, numpy's draws, outputs numpy consumed) of PCG64(seed)."""
    raw = np.random.PCG64(seed).random_raw(count + count // 16 + 64)
    bg = np.random.PCG64(seed)
    draws = np.random.Generator(bg).standard_normal(count)
    return raw, draws, bg


@pytest.mark.parametrize("seed", [0, 12345, 1000000 * (18 * 3 + 7) + 4242])
def test_restatement_equals_numpy_draws_and_state(seed):
    count = 1 << 22
    raw, draws, bg = _raw_and_draws(seed, count)
    got, consumed, events = nr.normals_from_raw(raw, count, TABS)
    assert got.tobytes() == draws.tobytes()
    ref = np.random.PCG64(seed)
    ref.advance(consumed)
    assert ref.state == bg.state
    kinds = [e[1] for e in events]
    assert {nr.WEDGE, nr.REJECT, nr.TAIL} <= set(kinds)
    assert 0.9 < len(events) / (count * 0.01455) < 1.1  # wedges and tails: 1.455 % of the attempts leave the fast path


def test_committed_tables_are_the_installed_numpys():
    """wi and ki are compared with == for all 256 idx: a crafted state with rabs = 1 returns wi[idx] itself; rabs = ki - 1 consumes one
    output and rabs = ki more than one.  fi enters numpy's draw only through the wedge comparison, which no probe isolates: it is held
    to exp(-x^2 / 2) at the layer edges x = 2^52 wi[idx] within 1 ulp, and by the bulk comparison of the test above (2^22 draws of three
    seeds hold 1.8e5 wedge comparisons)."""
    wi, ki, fi = TABS

    def probe(idx, rabs):
        bg = nr.crafted_pcg64(nr.word(idx, 0, rabs))
        before = bg.state["state"]["state"]
        val = np.random.Generator(bg).standard_normal()
        after = bg.state["state"]["state"]
        one = (before * nr.MULT + bg.state["state"]["inc"]) & nr.M128
        return val, after == one

    for idx in range(256):
        val, single = probe(idx, 1)
        if int(ki[idx]) > 1:
            assert single and val == wi[idx], idx
        k = int(ki[idx])
        if k > 0:
            val, single = probe(idx, k - 1)
            assert single and val == (k - 1) * wi[idx], idx
        assert not probe(idx, k)[1], idx
    assert fi[0] == 1.0 and np.all(np.diff(fi) < 0)
    for idx in range(1, 256):
        x = float(wi[idx]) * 2.0**52
        assert abs(fi[idx] - math.exp(-0.5 * x * x)) <= np.spacing(fi[idx]), idx


def test_tool_reproduces_the_committed_header():
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ziggurat_tables.py"), "--check"]).returncode == 0


def _write_case(path, raw, count):
    draws, consumed, events = nr.normals_from_raw(raw, count, TABS)
    with open(path, "wb") as f:
        f.write(np.array([len(raw), count, consumed], dtype=np.int64).tobytes())
        f.write(np.asarray(raw, dtype=np.uint64).tobytes())
        f.write(draws.tobytes())
    return events


def test_native_core_equals_the_restatement_under_sanitizers(tmp_path):
    """Tile sizes 4 .. 2048 on: a stream of PCG64 (wedges, rejections and tails at every offset within a tile), and a crafted sequence of
    outputs in which a wedge, a rejection and a tail loop of four pairs each start on the last position of a 2048-tile, and so cross the
    end of every smaller tile too."""
    exe = tmp_path / "ziggurat_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "pyimcom_amd", "csrc"), os.path.join(ROOT, "tests", "native", "ziggurat_check.cpp"), "-o", str(exe)])
    wi, ki, fi = TABS
    count = 20000
    raw = np.random.PCG64(77).random_raw(count + 2048)
    ev = _write_case(tmp_path / "stream.bin", raw, count)
    assert {nr.WEDGE, nr.REJECT, nr.TAIL} <= {e[1] for e in ev}

    fast = nr.word(5, 0, 1000)
    u_word = lambda u: int(u * 2.0**53) << 11  # noqa: E731
    crafted = [fast] * (3 * 2048 + 64)
    idx = 100
    # a wedge accepted (u = 0: the left side is fi[idx], below exp(-x^2/2) inside the layer) from the last position of tile 0
    crafted[2047] = nr.word(idx, 1, int(ki[idx]) + 5)
    crafted[2048] = u_word(0.0)
    # a wedge refused (u close to 1) from the last position of tile 1, then a fresh attempt
    crafted[4095] = nr.word(idx, 0, nr.MASK52)
    crafted[4096] = u_word(1.0 - 2.0**-53)
    # a tail of four pairs from the last position of tile 2: three pairs refused (xx large, yy small), the fourth taken
    crafted[6143] = nr.word(0, 0, int(ki[0]) + (1 << 8))
    for pair in range(3):
        crafted[6144 + 2 * pair] = u_word(1.0 - 2.0**-30)
        crafted[6145 + 2 * pair] = u_word(2.0**-30)
    crafted[6150] = u_word(0.25)
    crafted[6151] = u_word(0.9)
    ev = _write_case(tmp_path / "crafted.bin", crafted, 3 * 2048 + 20)
    assert [(e[0], e[1], e[2]) for e in ev] == [(2047, nr.WEDGE, 2), (4095, nr.REJECT, 2), (6143, nr.TAIL, 9)]
    empty = _write_case(tmp_path / "empty.bin", crafted[:64], 0)
    assert empty == []

    out = subprocess.run([str(exe), str(tmp_path / "stream.bin"), str(tmp_path / "crafted.bin"), str(tmp_path / "empty.bin")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.strip().splitlines()]
    assert [r[1] for r in rows] == ["10", "10", "10"]
    assert rows[1][2:] == ["3", "1"] and rows[2][2:] == ["0", "0"]
