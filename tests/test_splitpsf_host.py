"""Host side of pyimcom_amd.splitpsf (no GPU): the numpy / scipy restatement tests/splitpsf_reference.py pinned to what the reference's
own code produced (tests/golden/splitpsf.npz, tests/golden/make_golden_splitpsf.py), the package's host helpers (Gauss-Legendre grid,
Legendre values, Jacobian, covariances: numpy only) against the same fixture, the routes and sizes the library reports, and the imports of
the package."""

import os
import subprocess
import sys

import numpy as np
import pytest

from tests import splitpsf_reference as ref
from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "splitpsf.npz")
CASES = ["a", "b", "c"]
OUTPUTS = ["psfcube", "smallpsf", "K_Legendre", "K_real", "zeta_real"]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def sp():
    import __graft_entry__ as g

    g.build()
    from pyimcom_amd import splitpsf

    return splitpsf


def pars_of(gold, name):
    pre = f"{name}_par_"
    return {k[len(pre):]: gold[k].item() for k in gold.files if k.startswith(pre)}


def build_kw(p):
    return dict(oversamp=p["oversamp"], r_in=p["r_in"], r_out=p["r_out"], eps=p["eps"], m_trunc=p.get("m_trunc", 0), smallstamp_size=p.get("smallstamp_size"))


def test_golden_holds_the_cases_of_the_issue(gold, sp):
    a, b, c = (pars_of(gold, n) for n in CASES)
    assert not gold["a_wcs"] and a["tophat_in"] and a.get("m_trunc", 0) == 0 and gold["a_cube"].shape[0] == 4
    assert sp.routes(gold["a_cube"].shape[1], a["oversamp"])[1] == sp.ROUTE_LINES
    assert gold["b_wcs"] and not b["tophat_in"] and b["m_trunc"] > 0 and b["smallstamp_size"] < gold["b_cube"].shape[1] and gold["b_cube"].shape[0] == 9
    assert sp.routes(gold["b_cube"].shape[1], b["oversamp"])[0] == sp.ROUTE_DENSE  # n + 2 npad has a prime factor above 5
    cov = gold["b_Cov"]
    assert np.abs(cov[:, 0, 1]).min() > 1e-3 * cov[:, 0, 0].max() and np.ptp(cov[:, 0, 0]) > 1e-6 * cov[:, 0, 0].max()  # sheared, varying
    assert not c["tophat_in"] and sp.routes(gold["c_cube"].shape[1], c["oversamp"])[0] == sp.ROUTE_LINES
    for n in CASES:
        assert gold[f"{n}_ref_err"].shape == (5,) and np.all(gold[f"{n}_ref_err"] < 1e-13 * np.abs(gold[f"{n}_psfcube"]).max())
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference(gold, name):
    p = pars_of(gold, name)
    cube = gold[f"{name}_cube"]
    filt = cube.copy() if p["tophat_in"] else ref.tophatfilter(cube, p["oversamp"])
    out = ref.build(filt, gold[f"{name}_Cov"], **build_kw(p))
    out["psfcube"] = filt
    for k, e in zip(OUTPUTS, gold[f"{name}_ref_err"]):
        d = np.abs(out[k] - gold[f"{name}_{k}"]).max()
        scale = gold[f"{name}_locmax"] if k == "zeta_real" else gold[f"{name}_{k}"]
        print(f"{name} {k}: |restatement - reference| {d:.3e}, bound {ref.bound(e, scale):.3e}")
        assert out[k].shape == gold[f"{name}_{k}"].shape and d <= ref.bound(e, scale)
    assert np.abs(out["locLRP"]).max() == float(gold[f"{name}_locmax"])
    # the extended-precision evaluation is what ref_err was measured against
    ext = ref.build(filt, gold[f"{name}_Cov"], extended=True, **build_kw(p))
    assert np.abs(ext["K_real"] - gold[f"{name}_K_real"]).max() <= 2 * gold[f"{name}_ref_err"][3] + 1e-300


@pytest.mark.parametrize("name", CASES)
def test_host_helpers_match_scipy_and_the_reference(gold, sp, name):
    p = pars_of(gold, name)
    npoly = gold[f"{name}_cube"].shape[0]
    lorder = int(round(np.sqrt(npoly))) - 1
    xg, yg, wg = sp.gauss_legendre_grid(lorder)
    np.testing.assert_allclose(np.stack([xg, yg, wg]), gold[f"{name}_grid"], rtol=1e-14, atol=0)
    np.testing.assert_allclose(sp.legendre_weights(lorder, xg, yg), gold[f"{name}_lpw"], rtol=1e-14, atol=1e-15)
    wcs_ = ref.ShearWCS() if gold[f"{name}_wcs"] else None
    cov = sp.covariances(wcs_, lorder, oversamp=p["oversamp"], sigmaGamma=p["sigmaGamma"], nside=p.get("nside", 4088),
                         ref_pixscale=p.get("ref_pixscale", 0.11))
    np.testing.assert_allclose(cov, gold[f"{name}_Cov"], rtol=1e-14, atol=1e-14 * np.abs(gold[f"{name}_Cov"]).max())


def test_sizes_and_routes(sp):
    from pyimcom_amd._lib import lib, ptr

    sz = np.zeros(6, dtype=np.int64)
    assert lib.imcom_splitpsf_sizes(512, 16, 8.0, 18, 16, ptr(sz)) == 0
    assert list(sz[:4]) == [8, 528, sp.ROUTE_DENSE, sp.ROUTE_LINES]  # 528 = 16 x 3 x 11; 1024
    planes, N = 18 * 16, 1024
    assert sz[5] >= planes * (2 * N * N * 16 + 2 * 512 * 512 * 8)  # two complex planes, locLRP and K_real per grid point and SCA
    assert lib.imcom_splitpsf_sizes(384, 16, 8.0, 1, 1, ptr(sz)) == 0 and list(sz[1:4]) == [400, sp.ROUTE_LINES, sp.ROUTE_LINES]
    assert lib.imcom_splitpsf_sizes(520, 16, 8.0, 1, 1, ptr(sz)) == 0 and sz[3] == sp.ROUTE_DENSE  # 2n = 1040 > 1024: the dense route
    assert lib.imcom_splitpsf_sizes(2050, 16, 8.0, 1, 1, ptr(sz)) == 0 and sz[3] == 0 and sz[5] == 0  # 2n > 4096: not served
    assert lib.imcom_splitpsf_sizes(512, 16, 8.0, 1, 17, ptr(sz)) == -1
    # a single sample is a side imcom_splitpsf_tophat takes (9 = 3 x 3 with a tophat of width 1: the smallest odd butterfly side)
    assert lib.imcom_splitpsf_sizes(1, 3, 1.0, 1, 1, ptr(sz)) == 0 and list(sz[:3]) == [4, 9, sp.ROUTE_LINES] and sz[4] > 0
    assert lib.imcom_splitpsf_sizes(0, 3, 1.0, 1, 1, ptr(sz)) == -1


def test_package_does_not_import_scipy_or_the_tests():
    code = ("import sys; import pyimcom_amd.splitpsf; "
            "bad = [m for m in sys.modules if m.split('.')[0] in ('scipy', 'oracle', 'tests')]; print(bad); sys.exit(1 if bad else 0)")
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout, out.stderr[-500:])
