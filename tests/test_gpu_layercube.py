"""Seam 23 on the GPU: ``imcom_layer_place`` against numpy computed here, ``pyimcom_amd.layers.build_cube`` / ``get_all_data`` against the
cubes the reference's own ``get_all_data`` produced (tests/golden/layercube.npz), one production-size cube against the dedicated seams,
the two consumers of the cube, the refusals and ``CubeCache``.  Every comparison is == on float32 bits (NaN where NaN)."""

import types
import warnings

import numpy as np
import pytest

from tests import layercube_reference as LR

pytestmark = pytest.mark.gpu

G, META = LR.load_golden()
N = META["nside"]
CASES = {c["name"]: c for c in META["cases"]}
SUB = 86.123456789
DTYPES = ["f4", "f8", "i2", "u2", "i4", "u1"]
CODE = {"f4": 0, "f8": 1, "i2": 2, "u2": 3, "i4": 4, "u1": 5}


def source_array(rng, dtype, order, ny, nx):
    """A source image of the dtype in the byte order: sky-like floats with NaN, both infinities and -0.0 in the window of every crop, or
    integers over the type's whole range."""
    dt = np.dtype(order + dtype) if dtype != "u1" else np.dtype("u1")
    if dtype in ("f4", "f8"):
        a = SUB + 12.0 * rng.standard_normal((ny, nx))
        a[5, 5:9] = (np.nan, np.inf, -np.inf, -0.0)
        a[6, 5] = 1.0e300 if dtype == "f8" else 3.0e38  # float64: beyond float32
        with np.errstate(over="ignore"):
            return a.astype(dt)
    info = np.iinfo(np.dtype(dtype))
    a = rng.integers(info.min, info.max, (ny, nx), endpoint=True)
    a[5, 5:7] = (info.min, info.max)
    return a.astype(dt)


def call_place(arr, nside, origin=(0, 0), flip=0, sub=None, scale=None, host=False, fill=np.nan):
    """imcom_layer_place on the bytes of ``arr`` as they are: from device memory (the raw bytes uploaded), or with ``host`` from host memory
    into a host plane.  Returns (status, plane as numpy)."""
    import torch

    from pyimcom_amd import _lib
    from pyimcom_amd._dev import bound_context

    ctx = bound_context("cuda:0")
    arr = np.ascontiguousarray(arr)
    args = (CODE[arr.dtype.str[1:]], 0 if arr.dtype.isnative else 1, arr.shape[0], arr.shape[1], origin[0], origin[1], flip, 0 if sub is None else 1,
            0.0 if sub is None else sub, 0 if scale is None else 1, 0.0 if scale is None else scale)
    if host:
        dst = np.full((nside, nside), fill, dtype=np.float32)
        rc = _lib.lib.imcom_layer_place(ctx.handle, _lib.ptr(arr), *args, _lib.ptr(dst), nside, _lib.MEM_HOST)
        return rc, dst
    src = torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    dst = torch.full((nside, nside), fill, dtype=torch.float32, device="cuda:0")
    rc = _lib.lib.imcom_layer_place(ctx.handle, _lib.ptr(src), *args, _lib.ptr(dst), nside, _lib.MEM_DEVICE)
    return rc, dst.cpu().numpy()


@pytest.mark.parametrize("nside", [24, 67, 257])
def test_layer_place_equals_numpy(nside):
    """Each dtype x byte order x flip x crop, plain, minus the sky, times 2.5, and minus the sky times 0.1; device sources throughout and
    host sources for one flip of each."""
    rng = np.random.default_rng(nside)
    planes = 0
    for dtype in DTYPES:
        for order in ("<", ">") if dtype != "u1" else ("|",):
            for grow, origin in ((0, (0, 0)), (4, (4, 4)), (8, (4, 4))):
                arr = source_array(rng, dtype, order, nside + grow, nside + grow)
                for flip in (0, 1, 2):
                    for sub, scale in ((None, None), (SUB, None), (None, 2.5), (SUB, 0.1)):
                        want = LR.bits(LR.place(arr, nside, origin, flip, sub, scale))
                        for host in (False, True) if flip == DTYPES.index(dtype) % 3 else (False,):
                            rc, got = call_place(arr, nside, origin, flip, sub, scale, host=host)
                            assert rc == 0
                            assert np.array_equal(LR.bits(got), want), (dtype, order, origin, flip, sub, scale, host)
                            planes += 1
    assert planes >= 11 * 3 * 3 * 4


def test_layer_place_keeps_nan_infinities_and_signed_zero():
    arr = np.array([[np.nan, np.inf, -np.inf, -0.0], [0.0, 1.0e-45, 3.0e38, -3.0e38], [1.0, 2.0, 3.0, 4.0], [5.0, 6.0, 7.0, 8.0]], dtype=">f4")
    for a in (arr, arr.astype(">f8"), arr.astype("<f8")):
        for sub, scale in ((None, None), (SUB, None), (None, 0.1)):
            rc, got = call_place(a, 4, sub=sub, scale=scale)
            want = LR.place(a, 4, subtract=sub, scale=scale)
            assert rc == 0 and np.array_equal(LR.bits(got), LR.bits(want))
            assert np.isnan(got[0, 0]) and got[0, 1] == np.inf and got[0, 2] == -np.inf
            if sub is None:
                assert np.signbit(got[0, 3]) and got[0, 3] == 0.0 and not np.signbit(got[1, 0])


def test_layer_place_refuses_bad_arguments_and_writes_nothing():
    from pyimcom_amd import _lib
    from pyimcom_amd._dev import bound_context
    import torch

    ctx = bound_context("cuda:0")
    src = torch.arange(12 * 12, dtype=torch.float32, device="cuda:0")
    dst = torch.full((8, 8), 7.0, dtype=torch.float32, device="cuda:0")
    good = dict(src_type=0, src_swapped=0, src_ny=12, src_nx=12, y0=4, x0=4, flip=0, op=0, sub=0.0, post=0, scale=0.0, nside=8, mem=1)

    def run(**change):
        a = dict(good, **change)
        return _lib.lib.imcom_layer_place(ctx.handle, _lib.ptr(a.get("src", src)), a["src_type"], a["src_swapped"], a["src_ny"], a["src_nx"], a["y0"], a["x0"], a["flip"],
                                          a["op"], a["sub"], a["post"], a["scale"], _lib.ptr(a.get("dst", dst)), a["nside"], a["mem"])

    bad = [dict(src_type=-1), dict(src_type=6), dict(src_swapped=2), dict(src_swapped=-1), dict(flip=3), dict(flip=-1), dict(op=2), dict(op=-1), dict(post=2),
           dict(nside=-1), dict(src_ny=-12), dict(src_nx=-12), dict(src_nx=65537), dict(y0=-1), dict(x0=-1), dict(y0=5), dict(x0=5), dict(nside=9), dict(src_ny=11),
           dict(src_nx=11), dict(src=None), dict(dst=None), dict(mem=2)]
    for change in bad:
        assert run(**change) == -1, change  # IMCOM_ERR_ARG
        assert _lib.lib.imcom_last_error()
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all())
    assert run() == 0 and np.array_equal(dst.cpu().numpy(), src.cpu().numpy().reshape(12, 12)[4:, 4:])
    assert run(nside=0, src_ny=0, src_nx=0, y0=0, x0=0, src=None, dst=None) == 0  # an empty plane is a no-op


# ---- the golden cases ------------------------------------------------------------------------------------------------------------------

def _cfg(case):
    return types.SimpleNamespace(n_inframe=len(case["extrainput"]), extrainput=case["extrainput"], informat=case["informat"], inpsf_oversamp=8,
                                 inlayercache="cache/cube" if case["inlayercache"] else None, cr_mask_rate=0.0)


def _to_device(a):
    import torch

    a = np.asarray(a)
    return torch.as_tensor(np.ascontiguousarray(a.astype(a.dtype.newbyteorder("=")))).to("cuda:0")


@pytest.mark.parametrize("on_device", [False, True], ids=["host_sources", "device_sources"])
@pytest.mark.parametrize("name", sorted(c for c in CASES if not CASES[c]["inlayercache"]))
def test_build_cube_equals_the_reference_cube(name, on_device, capsys):
    import torch

    from pyimcom_amd import layers

    case, calls = CASES[name], []

    def grid_image(res):
        calls.append(res)
        return _to_device(G["bright"]) if on_device else G["bright"]

    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        cube = layers.build_cube(_cfg(case), case["idsca"], LR.make_sources(G, case, layers.pick_noise_slice, _to_device if on_device else (lambda a: a)),
                                 grid_image=grid_image, galsim_layers=LR.make_galsim(G, case), nside=N)
    assert cube.dtype == torch.float32 and cube.is_cuda and tuple(cube.shape) == G["cube_" + name].shape
    got = cube.cpu().numpy()
    for i in range(got.shape[0]):
        assert np.array_equal(LR.bits(got[i]), LR.bits(G["cube_" + name][i])), (name, i, case["extrainput"][i])
    assert sorted(str(x.message) for x in w) == sorted(case["warnings"])
    assert capsys.readouterr().out.count("labnoise file not found") == case["labnoise_missing"]
    # the reference makes the star image once per layer that uses it; here once per cube, and the bits are the same
    assert len(calls) == min(1, case["grid_calls"])


@pytest.mark.parametrize("device_out", [False, True])
@pytest.mark.parametrize("name", ["cache_hit", "cache_miss", "dc2_f4"])
def test_get_all_data_with_in_memory_hooks(name, device_out):
    import torch

    from pyimcom_amd import layers

    case = CASES[name]
    inimage = types.SimpleNamespace(blk=types.SimpleNamespace(cfg=_cfg(case), obsdata=None), idsca=tuple(case["idsca"]), inwcs=None, get_psf_pos=None, indata=None)
    log = []

    def load_cached(im):
        log.append("load")
        return G["cached"] if case["inlayercache"] == "hit" else None

    def save_cached(im, host_cube):
        assert isinstance(host_cube, np.ndarray) and host_cube.dtype == np.float32
        log.append(("save", LR.bits(host_cube)))

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        layers.get_all_data(inimage, device_out=device_out, sources=LR.make_sources(G, case, layers.pick_noise_slice), load_cached=load_cached, save_cached=save_cached,
                            grid_image=lambda res: G["bright"], nside=N)
    got = inimage.indata
    assert (isinstance(got, torch.Tensor) and got.is_cuda) if device_out else isinstance(got, np.ndarray)
    got = got.cpu().numpy() if device_out else got
    assert got.dtype == np.float32 and np.array_equal(LR.bits(got), LR.bits(G["cube_" + name]))
    if case["inlayercache"] == "hit":
        assert log == ["load"]
    elif case["inlayercache"] == "miss":
        assert log[0] == "load" and len(log) == 2 and np.array_equal(log[1][1], LR.bits(G["cube_" + name]))
    else:
        assert log == []


# ---- one production-size cube ----------------------------------------------------------------------------------------------------------

def test_production_size_cube_plane_by_plane():
    import torch

    from pyimcom_amd import inject, layers, noiselayers

    nside, idsca = 4088, (1234, 5)
    names = ["", "whitenoise1", "1fnoise2", "labnoise", "nstar14,2e5,86,3", "cstar14"]
    rng = np.random.default_rng(4088)
    sci = (SUB + 12.0 * rng.standard_normal((nside, nside), dtype=np.float32)).astype(">f4")
    lab = (3.0 * rng.standard_normal((4096, 4096), dtype=np.float32)).astype(">f4")
    made = []

    def grid_image(res):  # unit-flux spots at a 64-pixel pitch on a slightly negative floor, float64 on the device
        made.append(res)
        t = torch.arange(nside, dtype=torch.float64, device="cuda:0")
        d = (t % 64.0 - 31.5) ** 2
        return torch.exp(-0.5 * (d[:, None] + d[None, :]) / 2.25) / (2 * np.pi * 2.25) - 2.0e-5

    cfg = types.SimpleNamespace(n_inframe=len(names), extrainput=names, informat="dc2_imsim", inpsf_oversamp=8)
    cube = layers.build_cube(cfg, idsca, lambda kind, label=None: {"sci": (sci, SUB), "labnoise": lab}.get(kind), grid_image=grid_image, nside=nside)
    assert made == [14] and tuple(cube.shape) == (6, nside, nside) and cube.dtype == torch.float32

    def same(plane, want):
        if isinstance(want, np.ndarray):
            want = torch.from_numpy(np.ascontiguousarray(want)).to("cuda:0")
        return bool(((plane == want) | (torch.isnan(plane) & torch.isnan(want))).all()) and plane.dtype == want.dtype == torch.float32

    assert same(cube[0], sci - SUB)  # numpy: float32 - float32(sky)
    assert same(cube[1], np.random.default_rng(layers.layer_seed(1, idsca)).normal(loc=0.0, scale=1.0, size=(nside, nside)).astype(np.float32))
    assert same(cube[2], noiselayers.noise_1f_frame(layers.layer_seed(2, idsca), device_out=True))
    assert same(cube[3], lab[4:4092, 4:4092].astype(np.float32))
    b = grid_image(14)
    assert same(cube[4], inject.nstar_layer(b, 2.0e5, 86.0, 3, idsca, device_out=True))
    assert same(cube[5], b.cpu().numpy().astype(np.float32))
    assert bool((b < 0).any()) and float(cube[4].std()) > 1.0


# ---- the consumers ---------------------------------------------------------------------------------------------------------------------

def _small_cube(nside, names=("", "labnoise", "whitenoise2", "truth,2.5")):
    from pyimcom_amd import layers

    rng = np.random.default_rng(nside)
    src = {"sci": ((SUB + rng.standard_normal((nside, nside))).astype(">f4"), SUB), "truth": rng.integers(0, 1000, (nside, nside)).astype(">i2"),
           "labnoise": (2.0 * rng.standard_normal((nside + 8, nside + 8))).astype(">f4")[4:-4, 4:-4]}  # a strided view of a larger image
    cfg = types.SimpleNamespace(n_inframe=len(names), extrainput=list(names), informat="anlsim", inpsf_oversamp=8)
    return layers.build_cube(cfg, (1234, 5), lambda kind, label=None: src.get(kind), nside=nside), src


def test_extract_layers_takes_the_device_cube():
    from tests import test_gpu_inpool as TI

    name, key, masked = next(v for v in TI.VARIANTS if TI.META["images"][v[0]]["is_relevant"])
    part = TI.cached(name, key, masked)
    cube, src = _small_cube(TI.NSIDE)
    assert not src["labnoise"].flags.c_contiguous  # (a non-contiguous source went in)
    assert np.array_equal(LR.bits(cube[1].cpu().numpy()), LR.bits(src["labnoise"].astype(np.float32)))
    dev, host = part.extract_layers(cube), part.extract_layers(cube.cpu().numpy())
    assert dev.is_cuda and dev.shape[0] == 4 and np.array_equal(LR.bits(dev.cpu().numpy()), LR.bits(host.cpu().numpy())) and bool(dev.any())


def test_load_cr_mask_takes_the_device_cube():
    from pyimcom_amd import simmask

    cube, _ = _small_cube(67)
    cfg = types.SimpleNamespace(cr_mask_rate=0.02, extrainput=[None, "labnoise", "whitenoise2", "truth,2.5"], labnoisethreshold=1.5)
    masks = []
    for indata in (cube, cube.cpu().numpy()):
        masks.append(simmask.load_cr_mask(types.SimpleNamespace(blk=types.SimpleNamespace(cfg=cfg), idsca=(1234, 5), indata=indata)))
    assert masks[0].dtype == np.bool_ and masks[0].shape == (67, 67) and np.array_equal(masks[0], masks[1])
    assert 0 < masks[0].sum() < 67 * 67 and not masks[0][np.abs(cube[1].cpu().numpy()) >= 1.5].any()


# ---- errors ----------------------------------------------------------------------------------------------------------------------------

def _build(names, sources=None, informat="dc2_imsim", nside=N, **kw):
    from pyimcom_amd import layers

    cfg = types.SimpleNamespace(n_inframe=len(names), extrainput=names, informat=informat, inpsf_oversamp=8)
    return layers.build_cube(cfg, (1234, 5), sources or (lambda kind, label=None: None), nside=nside, **kw)


def test_errors():
    from pyimcom_amd import _lib

    for name in ("gsstar14", "gsextchrom14,path"):
        try:
            import pyimcom.layer  # noqa: F401  (with the reference and GalSim at hand the default provider would draw)
        except ImportError:
            with pytest.raises(_lib.ImcomError) as e:
                _build([None, name])
            assert e.value.status == -4 and name in str(e.value)  # IMCOM_ERR_UNSUPPORTED
    for shape in ((1, N), (N, 1), (1, 1), (1, N, N), (N + 1, N)):
        for kind, names in (("sci", [None]), ("labnoise", [None, "labnoise"]), ("truth", [None, "truth"])):
            with pytest.raises(ValueError):
                _build(names, lambda k, label=None, kind=kind, shape=shape: np.zeros(shape, dtype=np.float32) if k == kind else None)
    with pytest.raises(ValueError):  # the crop of a (26, 28) file is (22, 24)
        _build([None, "labnoise"], lambda k, label=None: np.zeros((N + 2, N + 4), dtype=np.float32) if k == "labnoise" else None)
    for bad in (np.zeros((N, N), dtype=np.complex64), np.zeros((N, N), dtype=np.int64), np.zeros((N, N), dtype=np.float16), np.zeros((N, N), dtype=bool)):
        with pytest.raises(TypeError):
            _build([None], lambda k, label=None, bad=bad: bad)
    with pytest.raises(ValueError):
        _build([None, "1fnoise3"])
    with pytest.raises(TypeError):
        _build([None, "cstar14"], grid_image=lambda res: np.zeros((N - 1, N)))


# ---- CubeCache on the device -----------------------------------------------------------------------------------------------------------

def test_cube_cache_on_the_device():
    import torch

    from pyimcom_amd.layers import CubeCache

    def cube(v):
        return torch.full((2, 1024, 1024), float(v), dtype=torch.float32, device="cuda:0")  # 8 MiB

    torch.cuda.synchronize()
    cache = CubeCache(max_bytes=12 << 20)
    base = torch.cuda.memory_allocated()
    a = cache.get((1, 1), lambda: cube(1))
    assert cache.get((1, 1), lambda: cube(-1)) is a and cache.bytes == 8 << 20
    del a
    b = cube(2)
    both = torch.cuda.memory_allocated()
    assert both - base >= 16 << 20
    assert cache.get((2, 1), lambda: b) is b and cache.keys() == [(2, 1)]  # (1, 1) does not fit beside it: evicted
    assert torch.cuda.memory_allocated() <= both - (8 << 20)
    cache.clear()
    del b
    assert torch.cuda.memory_allocated() <= base and cache.bytes == 0
