"""pyimcom_amd.splitpsf on the device (csrc/splitpsf.hip) against the reference's own outputs (tests/golden/splitpsf.npz, produced by
executing src/pyimcom/splitpsf/splitpsf.py's class: tests/golden/make_golden_splitpsf.py) and, for shapes too big to commit, against the
restatement tests/splitpsf_reference.py that tests/test_splitpsf_host.py pins to the same fixture.

Tolerance.  The fixture stores per case and output ref_err = max |reference - the same arithmetic with extended-precision transforms|.
The device must lie within max(10 ref_err, 2e-13 max |reference|) of the reference for psfcube (after the tophat filter), smallpsf,
K_real, K_Legendre and zeta_real (the latter on the scale of max |locLRP|: zeta is a difference of nearly equal terms).  The factor 10
covers another factorisation of the transforms and FMA contraction; 2e-13 is the table tolerance of tests/parity.py.  Every test prints
the distances it found before it asserts.  Nothing is masked."""

import os

import numpy as np
import pytest

from tests import splitpsf_reference as ref
from tests.conftest import ROOT
from tests.test_splitpsf_host import CASES, OUTPUTS, build_kw, pars_of

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "splitpsf.npz")
F32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def sp():
    import __graft_entry__ as g

    g.build()
    from pyimcom_amd import splitpsf

    return splitpsf


def _wcs(gold, name):
    return ref.ShearWCS() if gold[f"{name}_wcs"] else None


def _check(label, got, want, ref_err, scale=None):
    d = float(np.abs(np.asarray(got) - want).max())
    b = ref.bound(ref_err, want if scale is None else scale)
    print(f"{label}: |device - reference| {d:.3e}  bound {b:.3e}  (ref_err {float(ref_err):.3e}, max |reference| {np.abs(want).max():.3e})")
    assert np.asarray(got).shape == want.shape and np.asarray(got).dtype == np.float64
    assert d <= b


def _check_all(gold, name, obj):
    for k, e in zip(OUTPUTS, gold[f"{name}_ref_err"]):
        got = getattr(obj, k)
        got = got.cpu().numpy() if hasattr(got, "cpu") else got
        _check(f"{name} {k}", got, gold[f"{name}_{k}"], e, gold[f"{name}_locmax"] if k == "zeta_real" else None)
    np.testing.assert_allclose(obj.Cov, gold[f"{name}_Cov"], rtol=1e-14, atol=1e-14 * np.abs(gold[f"{name}_Cov"]).max())
    assert abs(obj.maxzeta - gold[f"{name}_header"][0]) <= ref.bound(gold[f"{name}_ref_err"][4], gold[f"{name}_locmax"])


@pytest.mark.parametrize("name", CASES)
def test_golden_case_numpy_in(gold, sp, name):
    p = pars_of(gold, name)
    n = gold[f"{name}_cube"].shape[1]
    top, dec = sp.routes(n, p["oversamp"])
    print(f"{name}: tophat route {top if not p['tophat_in'] else '-'} (side {n} + 2 npad), deconvolution route {dec} (side {2 * n})")
    assert dec == sp.ROUTE_LINES and (p["tophat_in"] or top == {"b": sp.ROUTE_DENSE, "c": sp.ROUTE_LINES}[name])
    obj = sp.SplitPSF(gold[f"{name}_cube"], _wcs(gold, name), p).build()
    assert all(isinstance(getattr(obj, k), np.ndarray) for k in OUTPUTS)
    _check_all(gold, name, obj)


@pytest.mark.parametrize("name", CASES)
def test_golden_case_torch_in_stays_on_the_device(gold, sp, name):
    import torch

    p = pars_of(gold, name)
    cube = torch.as_tensor(gold[f"{name}_cube"], device="cuda:0")
    obj = sp.SplitPSF(cube, _wcs(gold, name), p).build()
    for k in OUTPUTS:
        t = getattr(obj, k)
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64
    _check_all(gold, name, obj)
    # keep=(): the stacks are not materialised, max |zeta| is there all the same; K_Legendre is the same bit for bit
    lean = sp.SplitPSF(cube, _wcs(gold, name), p).build(keep=())
    assert not hasattr(lean, "K_real") and not hasattr(lean, "zeta_real") and lean.maxzeta == obj.maxzeta
    assert torch.equal(lean.K_Legendre, obj.K_Legendre)


@pytest.mark.parametrize("name", CASES)
def test_k_legendre_is_bit_identical_for_every_chunking(gold, sp, name):
    p = pars_of(gold, name)
    cube = gold[f"{name}_cube"]
    whole = sp.SplitPSF(cube, _wcs(gold, name), p).build()
    single = sp.SplitPSF(cube, _wcs(gold, name), p).build(points_per_call=1)
    for k in OUTPUTS:
        assert np.array_equal(getattr(whole, k), getattr(single, k)), k
    assert whole.maxzeta == single.maxzeta
    # three SCAs (the cube, scaled and flipped copies) in one call, one SCA per call, one grid point of one SCA per call
    cubes = np.stack([cube, 0.5 * cube[:, ::-1, :], 2.0 * cube[:, :, ::-1]])
    wl = [_wcs(gold, name), None, _wcs(gold, name)]
    a = sp.split_cubes(cubes, wl, p, sca_per_call=3)
    b = sp.split_cubes(cubes, wl, p, sca_per_call=1)
    c = sp.split_cubes(cubes, wl, p, sca_per_call=1, points_per_call=1)
    for k in ("smallpsf", "K_Legendre", "MAXZETA", "KINT", "K2INT"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
    assert np.array_equal(a["K_Legendre"][0], whole.K_Legendre.astype(np.float32))


@pytest.mark.parametrize("name", CASES)
def test_split_cubes_gives_the_file_contents(gold, sp, name):
    p = pars_of(gold, name)
    out = sp.split_cubes(gold[f"{name}_cube"][None], [_wcs(gold, name)], p)
    for k in ("smallpsf", "K_Legendre"):
        got, want = out[k][0], gold[f"{name}_{k}"].astype(np.float32)
        assert got.dtype == np.float32 and got.shape == want.shape
        for a in range(want.shape[0]):  # within one float32 ulp of the plane's maximum
            d, top = np.abs(got[a].astype(np.float64) - want[a].astype(np.float64)).max(), np.abs(want[a]).max()
            assert d <= F32 * top, (k, a, d, top)
    got, want = np.array([out["MAXZETA"][0], out["KINT"][0], out["K2INT"][0]]), gold[f"{name}_header"]
    print(f"{name} header: device {got}, reference {want}, relative {np.abs(got / want - 1)}")
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    assert out["TRUEWCS"].tolist() == [bool(gold[f"{name}_wcs"])]


def _full_cube(rng, npoly, n):
    X_ = np.linspace((1 - n) / 2.0, (n - 1) / 2.0, n)
    xx, yy = np.meshgrid(X_, X_)
    r2 = xx**2 + yy**2
    base = np.exp(-r2 / 50.0) + 0.05 / (1 + r2 / 40.0) ** 1.5
    cube = np.stack([(1.0 if a == 0 else 0.1 / (1 + a)) * base * (1 + 0.2 * rng.standard_normal((n, n))) for a in range(npoly)])
    return cube / cube[0].sum()


def _against_restatement(sp, cube, p, cov, points, label):
    """The device against tests/splitpsf_reference.py on the grid points ``points`` (K_real, zeta_real) with ref_err measured here the way
    tests/golden/make_golden_splitpsf.py measures it: every transform of the chain, the constructor's included, in extended precision."""
    filt = filt_ext = cube.copy()
    if not p.get("tophat_in"):
        filt, filt_ext = ref.tophatfilter(cube, p["oversamp"]), ref.tophatfilter(cube, p["oversamp"], extended=True)
    obj = sp.SplitPSF(cube, None, p, cov=cov).build()
    if not p.get("tophat_in"):
        _check(f"{label} psfcube", obj.psfcube, filt, np.abs(filt - filt_ext).max())
    kw = build_kw(p)
    want = ref.build(filt, cov, points=points, **kw)
    ext = ref.build(filt_ext, cov, points=points, extended=True, **kw)
    _check(f"{label} smallpsf", obj.smallpsf, want["smallpsf"], np.abs(want["smallpsf"] - ext["smallpsf"]).max())
    pts = list(points)
    for k, scale in (("K_real", None), ("zeta_real", np.abs(want["locLRP"]).max())):
        _check(f"{label} {k}", getattr(obj, k)[pts], want[k][pts], np.abs(want[k][pts] - ext[k][pts]).max(), scale)
    return obj, want, ext


def test_full_size_sca_against_the_restatement(sp):
    """16 planes of side 512 (transforms of 1024: butterflies; the tophat filter on 528 = 16 x 3 x 11: dense), distorted Cov."""
    rng = np.random.default_rng(5)
    cube = _full_cube(rng, 16, 512)
    p = dict(oversamp=8, r_in=4.0, r_out=9.0, sigmaGamma=1.0, eps=0.02, m_trunc=6, smallstamp_size=160)
    cov = sp.covariances(ref.ShearWCS(), 3, oversamp=8, sigmaGamma=1.0, nside=4088, ref_pixscale=0.11)
    assert sp.routes(512, 8) == (sp.ROUTE_DENSE, sp.ROUTE_LINES)
    obj, want, ext = _against_restatement(sp, cube, p, cov, (0, 6, 15), "full")
    # K_Legendre from the device's K_real with the reference's sum (277, 282-284): the accumulation itself is exact to the bit
    _, _, wg, lpw = ref.grid(3)
    KL = np.zeros_like(obj.K_Legendre)
    for i in range(16):
        KL += wg[i] * np.tensordot(lpw[i], obj.K_real[i], axes=0)
    l_ = np.arange(4) + 0.5
    KL = KL * np.outer(l_, l_).flatten()[:, None, None]
    host = sp.legendre_weights(3, *sp.gauss_legendre_grid(3)[:2])
    d = np.abs(obj.K_Legendre - KL).max()
    print(f"full K_Legendre: |device - numpy sum of the device's K_real| {d:.3e} (scipy vs numpy Legendre values {np.abs(host - lpw).max():.1e})")
    assert d <= 2e-13 * np.abs(KL).max()


def test_dense_route_of_the_deconvolution_and_sides_beyond_1024(sp):
    rng = np.random.default_rng(11)
    # 2n = 88 = 8 x 11: no butterfly plan
    assert sp.routes(44, 4)[1] == sp.ROUTE_DENSE
    cov = sp.covariances(ref.ShearWCS(), 1, oversamp=4, sigmaGamma=0.9, nside=4088, ref_pixscale=0.11)
    p = dict(oversamp=4, r_in=1.0, r_out=3.0, sigmaGamma=0.9, eps=0.03, tophat_in=True, m_trunc=2)
    obj, want, ext = _against_restatement(sp, _full_cube(rng, 4, 44), p, cov, range(4), "dense 88")
    _check("dense 88 K_Legendre", obj.K_Legendre, want["K_Legendre"], np.abs(want["K_Legendre"] - ext["K_Legendre"]).max())
    # 2n = 1028 > 1024: served by the dense route, one plane
    assert sp.routes(514, 8)[1] == sp.ROUTE_DENSE
    p = dict(oversamp=8, r_in=4.0, r_out=9.0, eps=0.02, tophat_in=True)
    cov = np.array([[[70.0, 3.0], [3.0, 60.0]]])
    obj, want, ext = _against_restatement(sp, _full_cube(rng, 1, 514), p, cov, range(1), "dense 1028")
    _check("dense 1028 K_Legendre", obj.K_Legendre, want["K_Legendre"], np.abs(want["K_Legendre"] - ext["K_Legendre"]).max())
    # beyond 4096 the library refuses
    from pyimcom_amd._lib import ImcomError

    with pytest.raises(ImcomError) as e:
        sp.SplitPSF(np.zeros((1, 2050, 2050)), None, dict(tophat_in=True)).build(points_per_call=1)
    assert e.value.status == -4


@pytest.mark.parametrize("n,width,N,waves", [(2, 3.0, 10, 12), (794, 8.0, 810, 11), (992, 2.5, 1000, 9), (1008, 6.5, 1024, 9)])
def test_tophat_on_the_line_route_at_the_edges_of_the_plan(sp, n, width, N, waves):
    """The transform side N = n + 2 npad at the edges of fft_line_plan (csrc/fft_plan_core.h; tests/test_fft_plan.py pins the lines per
    workgroup): 10 is the smallest side the filter can reach, 810 has six stages and 11 lines per workgroup, 1000 three radix-5 stages and
    9 lines, 1024 9 lines.  Three planes ride as two complex ones: 2 N lines, no multiple of the lines per workgroup, so the last workgroup
    is ragged.  Against the restatement, with its extended-precision yardstick."""
    from pyimcom_amd._lib import MEM_HOST, check, default_context, lib, ptr

    sz = sp._sizes(n, 3, width)
    assert (int(sz[1]), int(sz[2])) == (N, sp.ROUTE_LINES) and (2 * N) % waves != 0
    cube = np.random.default_rng(N).standard_normal((3, n, n))
    out = np.empty_like(cube)
    check(lib.imcom_splitpsf_tophat(default_context().handle, ptr(cube), 3, n, width, ptr(out), MEM_HOST))
    want = ref.tophatfilter(cube, width)
    _check(f"tophat N = {N}", out, want, np.abs(want - ref.tophatfilter(cube, width, extended=True)).max())


def test_value_errors_as_the_reference(sp):
    with pytest.raises(ValueError, match="SplitPSF requires even dimension"):
        sp.SplitPSF(np.zeros((4, 31, 31)), None, {})
    with pytest.raises(ValueError, match="SplitPSF requires even dimension"):
        sp.SplitPSF(np.zeros((4, 32, 32)), None, {"smallstamp_size": 15})
    with pytest.raises(ValueError, match="SplitPSF Legendre polynomial dimension error"):
        sp.SplitPSF(np.zeros((5, 32, 32)), None, {})
    with pytest.raises(ValueError, match="SplitPSF Legendre polynomial dimension error"):
        sp.split_cubes(np.zeros((2, 3, 32, 32)), None, {})
    from pyimcom_amd._lib import MEM_HOST, default_context, lib, ptr

    h = default_context().handle
    z = np.zeros((4, 8, 8))
    assert lib.imcom_splitpsf_split(h, ptr(z), 4, 7, 6, 4.0, 9.0, 0, ptr(z), ptr(z), MEM_HOST) == -1
    bad = np.array([[[1.0, 2.0], [2.0, 1.0]]] * 4)  # not positive definite
    assert lib.imcom_splitpsf_points(h, ptr(z), 1, 4, 8, 0, 4, ptr(np.eye(4)), ptr(np.ones(4)), ptr(bad), 0.02, ptr(z.copy()), None, None,
                                     ptr(np.zeros(1)), MEM_HOST) == -1


def test_host_staging_of_the_c_abi(gold, sp):
    """IMCOM_MEM_HOST: the three entries on numpy arrays give what the device-pointer path gives, bit for bit."""
    from pyimcom_amd._lib import MEM_HOST, check, default_context, lib, ptr

    name = "c"
    p = pars_of(gold, name)
    cube = gold[f"{name}_cube"]
    npoly, n, _ = cube.shape
    obj = sp.SplitPSF(cube, None, p).build()
    h = default_context().handle
    filt = np.empty_like(cube)
    check(lib.imcom_splitpsf_tophat(h, ptr(cube), npoly, n, float(p["oversamp"]), ptr(filt), MEM_HOST))
    assert np.array_equal(filt, obj.psfcube)
    small, resid = np.empty_like(cube), np.empty_like(cube)
    check(lib.imcom_splitpsf_split(h, ptr(filt), npoly, n, n, p["oversamp"] * p["r_in"], p["oversamp"] * p["r_out"], 0, ptr(small), ptr(resid), MEM_HOST))
    assert np.array_equal(small, obj.smallpsf)
    xg, yg, wg = sp.gauss_legendre_grid(1)
    lpw = sp.legendre_weights(1, xg, yg)
    KL, Kr, ze, zm = np.empty_like(cube), np.empty_like(cube), np.empty_like(cube), np.zeros(1)
    check(lib.imcom_splitpsf_points(h, ptr(resid), 1, npoly, n, 0, npoly, ptr(lpw), ptr(wg), ptr(np.ascontiguousarray(obj.Cov)), p["eps"], ptr(KL), ptr(Kr),
                                    ptr(ze), ptr(zm), MEM_HOST))
    assert np.array_equal(KL, obj.K_Legendre) and np.array_equal(Kr, obj.K_real) and np.array_equal(ze, obj.zeta_real) and zm[0] == obj.maxzeta


def test_float32_kernel_feeds_the_long_range_subtraction(gold, sp):
    """Stage 1 into stage 3: the float32 K_Legendre of split_cubes is what imsubtract.prepare_kernel / LongRangeSubtractor take (shape,
    dtype, plane order lu + lv Nl); the layer it subtracts differs from the one the reference's K subtracts by no more than the
    difference of the two kernels can make: sum |dK| max |canvas| max |P_l|^2 (the canvas reaches I_pad pixels beyond the SCA, where
    |u| > 1) plus one float32 rounding of the layer."""
    from pyimcom_amd import imsubtract

    name = "b"
    p = pars_of(gold, name)
    s = p["oversamp"]
    Kdev = sp.split_cubes(gold[f"{name}_cube"][None], [_wcs(gold, name)], p)["K_Legendre"][0]
    Kref = gold[f"{name}_K_Legendre"].astype(np.float32)
    ax = Kdev.shape[1]
    if ax % (2 * s):  # imsubtract.py:365-366 wants a multiple of 2 oversamp: the centred crop
        cut = (ax % (2 * s)) // 2
        Kdev, Kref = Kdev[:, cut:-cut, cut:-cut], Kref[:, cut:-cut, cut:-cut]
    K1, s1 = imsubtract.prepare_kernel(Kdev, s)
    assert s1 == s and K1.dtype == np.float32 and K1.shape == Kdev.shape and np.array_equal(K1, Kdev)
    nside = 24
    I_pad, _, A = imsubtract.geometry(K1.shape[1], s, nside)
    pmax = np.abs(np.polynomial.legendre.legvander(np.array([1.0 + 2.0 * I_pad / nside]), 2)).max()
    rng = np.random.default_rng(3)
    canvas = rng.standard_normal((A, A)).astype(np.float32)
    image = rng.standard_normal((nside, nside)).astype(np.float32)
    assert imsubtract.legendre_order(K1.shape[0]) == 3
    out_dev, kh_dev = imsubtract.subtract_long_range(image.copy(), canvas, K1, oversamp=s, nside=nside, return_kh=True)
    out_ref, kh_ref = imsubtract.subtract_long_range(image.copy(), canvas, Kref, oversamp=s, nside=nside, return_kh=True)
    dK = np.abs(K1.astype(np.float64) - Kref.astype(np.float64)).sum()
    d = np.abs(kh_dev - kh_ref).max()
    print(f"sum |dK| {dK:.3e}, |KH(device K) - KH(reference K)| {d:.3e}, bound {dK * np.abs(canvas).max() * pmax**2:.3e}")
    assert d <= dK * float(np.abs(canvas).max()) * pmax**2 + 1e-300
    assert np.abs(out_dev - out_ref).max() <= d + F32 * np.abs(image).max()
