"""Seam 23 on the host: the golden cubes that the reference's own ``get_all_data`` produced (tests/golden/make_golden_layercube.py) against
the numpy restatement (tests/layercube_reference.py), the host helpers of ``pyimcom_amd.layers`` (``layer_seed``, ``pick_noise_slice``,
``galsim_kind``, ``CubeCache``) and the host-compilable core of the kernel under the sanitizers.  Every comparison is on float32 bits."""

import os
import subprocess
import warnings

import numpy as np
import pytest

from tests import layercube_reference as LR
from tests.conftest import ROOT

G, META = LR.load_golden()
N = META["nside"]
CASES = {c["name"]: c for c in META["cases"]}


def _grid(res):
    assert res == 14
    return G["bright"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_reference_cube(name):
    case = CASES[name]
    if case["inlayercache"] == "hit":  # layer.py:1246: the cached cube, cast
        assert np.array_equal(LR.bits(G["cached"].astype(np.float32)), LR.bits(G["cube_" + name]))
        return
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        cube = LR.build_cube(case, LR.make_sources(G, case), N, grid_image=_grid, galsim_layers=LR.make_galsim(G, case))
    assert cube.dtype == np.float32 and cube.shape == G["cube_" + name].shape
    for i in range(cube.shape[0]):
        assert np.array_equal(LR.bits(cube[i]), LR.bits(G["cube_" + name][i])), (name, i, case["extrainput"][i])
    assert sorted(str(x.message) for x in w) == sorted(case["warnings"])


def test_golden_covers_what_it_should():
    """The fixture's own record: both flips, the crop path, the missing files, the unknown name and the byte orders are in it."""
    assert int(np.__version__.split(".")[0]) >= 2 and int(META["numpy"].split(".")[0]) >= 2
    assert G["sci_f4"].dtype.str == ">f4" and G["sci_f8"].dtype.str == ">f8" and G["sci_i2"].dtype.str == ">i2"
    assert CASES["anlsim_f8"]["cropped"] == 2 and CASES["l2_sca3"]["cropped"] == 1 and CASES["dc2_i2"]["labnoise_missing"] == 1
    assert not G["cube_dc2_f4"][9].any() and not G["cube_dc2_f4"][10].any() and not G["cube_missing_sci"][0].any()
    assert (G["bright"] < 0).mean() > 0.25 and CASES["dc2_f4"]["grid_calls"] == 2
    # SCA 3 reverses x, SCA 4 reverses y
    assert np.array_equal(G["cube_l2_sca3"][2], G["lab28"][4:28, 4:28].astype(np.float32)[:, ::-1])
    assert np.array_equal(G["cube_l2_sca4"][2], G["lab24"].astype(np.float32)[::-1, :])
    # gsextchrom<res> does not match ^gsext(\d+) (a digit must follow "gsext"): the reference makes one call for it
    assert [c[0] for c in CASES["galsim"]["galsim_calls"]] == ["extobj_grid", "star_grid", "star_grid", "star_grid", "extobj_grid", "extobj_grid"]
    assert CASES["cache_miss"]["saved"] == ["cache/cube_00001234_05.fits"]
    assert np.array_equal(LR.bits(G["cube_cache_miss"]), LR.bits(G["cube_dc2_f4"][:2]))


def test_layer_seed_is_the_reference_seed_and_the_one_inside_nstar_layer(monkeypatch):
    from pyimcom_amd import inject, layers, noiselayers

    assert CASES["dc2_f4"]["seeds"] == [layers.layer_seed(3, (1234, 5))] * 2  # whitenoise3 and nstar...,3
    assert CASES["anlsim_f8"]["seeds"] == [layers.layer_seed(3, (77, 3))]
    seen = []

    def capture(bitgen, offset, values, shape, *rest):
        seen.append(bitgen.state)
        return np.zeros(shape, dtype=np.float32), {}

    monkeypatch.setattr(noiselayers, "_poisson_call", capture)
    for q, idsca in ((3, (1234, 5)), (0, (1, 1)), (17, (99999, 18))):
        inject.nstar_layer(np.zeros((2, 2)), 2.0e5, 86.0, q, idsca)
        assert seen[-1] == np.random.PCG64(layers.layer_seed(q, idsca)).state


def test_pick_noise_slice_against_the_reference_warnings():
    from pyimcom_amd import layers

    case = CASES["l2_sca3"]
    labels, fname = case["sources"]["noise"][1], LR.noise_filename(case)
    got = []
    for label, want in (("b", 1), ("zz", -1), ("rep", 0)):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            assert layers.pick_noise_slice(labels, label, fname) == want == LR.pick(labels, label, fname)
        got += [str(x.message) for x in w][: len(w) // 2]  # (each helper warned once)
    assert got == case["warnings"]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert layers.pick_noise_slice([], "b", fname) == -1 and layers.pick_noise_slice(["b", "b", "b"], "b", fname) == 0
    assert len(w) == 2  # (the reference stops at the second instance: one warning, not two)


def test_galsim_kind_follows_the_reference_tests():
    from pyimcom_amd import layers

    names = CASES["galsim"]["extrainput"][1:]
    assert [layers.galsim_kind(n) for n in names] == ["gsextchrom", "gsstar", "gstrstar", "gsfdstar", "gsext", "gsext"]
    assert [layers.galsim_kind(n) for n in ("gsstar", "gsstar14x", "cstar14", "gsfdstar14", "truth", "")] == [None] * 6
    assert layers.flip_of("L2_2506", (1, 3)) == 1 and layers.flip_of("L2_2506", (1, 4)) == 2 and layers.flip_of("anlsim", (1, 3)) == 0


def test_cube_cache_order_bytes_oversize_and_clear():
    import torch

    from pyimcom_amd.layers import CubeCache

    made = []

    def maker(tag, n):
        def build():
            made.append(tag)
            return torch.full((n,), float(tag), dtype=torch.float32)
        return build

    cache = CubeCache(max_bytes=100 * 4)
    a = cache.get((1, 1), maker(1, 40))
    b = cache.get((2, 1), maker(2, 40))
    assert cache.bytes == 320 and cache.keys() == [(1, 1), (2, 1)]
    assert cache.get((1, 1), maker(-1, 40)) is a and made == [1, 2] and cache.keys() == [(2, 1), (1, 1)]  # a hit: no build, now the newest
    c = cache.get((3, 1), maker(3, 40))  # 120 elements do not fit: the least recently used, (2, 1), goes
    assert cache.keys() == [(1, 1), (3, 1)] and cache.bytes == 320
    assert cache.get((2, 1), maker(22, 100)) is not b and cache.keys() == [(2, 1)] and cache.bytes == 400  # exactly the budget: everything else goes
    big = cache.get((4, 1), maker(4, 101))  # larger than the budget: handed back, not kept, nothing evicted
    assert big.numel() == 101 and cache.keys() == [(2, 1)] and cache.bytes == 400
    assert cache.get((4, 1), maker(44, 101))[0] == 44.0  # (built again)
    assert cache.get([2, 1], maker(-1, 1))[0] == 22.0 and len(cache) == 1  # any (obsid, sca) pair is the key
    cache.clear()
    assert cache.bytes == 0 and len(cache) == 0 and c[0] == 3.0
    assert made == [1, 2, 3, 22, 4, 44]


def test_null_context_is_refused():
    from pyimcom_amd import _lib

    args = [0.0 if t is _lib._d else (0 if t in (_lib._i, _lib._l) else None) for t in _lib.SIGNATURES["imcom_layer_place"]]
    assert _lib.lib.imcom_layer_place(*args) == -1
    assert "null context" in _lib.lib.imcom_last_error().decode()


def test_native_core_against_plain_loops_under_sanitizers(tmp_path):
    exe = tmp_path / "layers_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(ROOT, "pyimcom_amd", "csrc"), os.path.join(ROOT, "tests", "native", "layers_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = dict(ln.split() for ln in out.stdout.strip().splitlines())
    # 6 sides x 6 types x 2 byte orders x 3 crops x (3 flips x 2 ops x 3 rescales)
    assert int(rows["planes"]) == 6 * 6 * 2 * 3 * 18 and int(rows["pixels"]) > 0 and int(rows["extents"]) == 13 and int(rows["refusals"]) == 16
    assert int(rows["mismatches"]) == 0
