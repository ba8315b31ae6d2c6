"""The plan of the wave-per-line FFT (pyimcom_amd/csrc/fft_plan_core.h) decides radices, table offsets, workgroup shapes and LDS sizes for
four seams.  It is host arithmetic: tests/native/fft_plan_check.cpp prints every plan (g++ with the address and undefined-behaviour
sanitizers), and every line is compared with a restatement of the rules written here, not taken from the C text."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXN, MAXST, MAXWAVES, LDS = 1024, 8, 12, 160 * 1024


def _tables(radix):
    """Stage s > 0 owns (radix[s] - 1) * Ns table values, Ns the product of the earlier radices; stage 0 has none."""
    twoff, off, ns = [0], 0, radix[0]
    for r in radix[1:]:
        twoff.append(off)
        off += (r - 1) * ns
        ns *= r
    return twoff, off


def _plan(n):
    """Greedy radices 16, 8, 4, 2, 3, 5; at least two stages; 6 <= n <= 1024; as many waves as 160 KiB hold beside the tables, 12 at most."""
    if not 6 <= n <= MAXN:
        return None
    radix, r = [], n
    for c in (16, 8, 4, 2, 3, 5):
        while r % c == 0:
            radix.append(c)
            r //= c
    if r != 1 or not 2 <= len(radix) <= MAXST:
        return None
    twoff, twn = _tables(radix)
    npad = -(-n // 16) * 16
    waves = min(MAXWAVES, (LDS - 16 * twn) // (16 * npad))
    if waves < 1:
        return None
    return dict(n=n, nst=len(radix), radix=radix, twoff=twoff, twn=twn, npad=npad, waves=waves, lds=(waves * npad + twn) * 16)


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fft_plan") / "fft_plan_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "pyimcom_amd", "csrc"), os.path.join(ROOT, "tests", "native", "fft_plan_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    plans = {"line": {}, "short": {}}
    for ln in out.stdout.strip().splitlines():
        f = ln.split()
        if f[2] == "none":
            plans[f[0]][int(f[1])] = None
            continue
        assert len(f) == 9, ln
        ints = lambda s: [int(v) for v in s.split(",")]  # noqa: E731
        plans[f[0]][int(f[1])] = dict(n=int(f[1]), nst=int(f[2]), radix=ints(f[3]), twoff=ints(f[4]), twn=int(f[5]), npad=int(f[6]),
                                      waves=int(f[7]), lds=int(f[8]))
    return plans


def test_every_side_against_the_restated_rules(printed):
    line = printed["line"]
    assert sorted(line) == list(range(2, MAXN + 1))
    for n in range(2, MAXN + 1):
        assert line[n] == _plan(n), n


def test_facts_of_the_plans(printed):
    line = {n: p for n, p in printed["line"].items() if p}
    assert len(line) == 80 and sorted(line)[:6] == [6, 9, 10, 12, 15, 18]
    assert not any(n in line for n in (4, 8, 16))
    assert max(p["nst"] for p in line.values()) == 6 < MAXST
    assert sorted(n for n, p in line.items() if p["nst"] == 6) == [486, 729, 810, 972]
    assert all(p["twn"] < n for n, p in line.items())  # the workspace take of n values holds the tables
    assert {n: p["waves"] for n, p in line.items() if p["waves"] != 12} == {800: 11, 810: 11, 864: 10, 900: 10, 960: 9, 972: 9, 1000: 9, 1024: 9}
    assert all(p["lds"] <= LDS and len(p["radix"]) == len(p["twoff"]) == p["nst"] for p in line.values())
    assert (line[768]["radix"], line[768]["twoff"], line[768]["twn"]) == ([16, 16, 3], [0, 0, 240], 752)
    assert (line[1000]["radix"], line[1000]["twoff"], line[1000]["twn"]) == ([8, 5, 5, 5], [0, 0, 32, 192], 992)
    assert (line[60]["radix"], line[60]["twn"]) == ([4, 3, 5], 56)


def test_short_plans_field_by_field(printed):
    """4, 8 and 16 as two stages for the noise spectra's sub-transforms: the values that seam used to fill in by hand -- radices {2,2},
    {4,2}, {4,4}, one slice of 16 values, one wave, both table offsets 0, twn = (r1 - 1) r0."""
    want = {4: ([2, 2], 2), 8: ([4, 2], 4), 16: ([4, 4], 12)}
    assert sorted(printed["short"]) == [4, 8, 16]
    for n, (radix, twn) in want.items():
        assert printed["short"][n] == dict(n=n, nst=2, radix=radix, twoff=[0, 0], twn=twn, npad=16, waves=1, lds=(16 + twn) * 16), n
        assert twn == (radix[1] - 1) * radix[0] and _tables(radix) == ([0, 0], twn)
