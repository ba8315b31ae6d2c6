"""The plumbing the seams share (pyimcom_amd/_dev.py): what is a tensor, dtype mapping, the value numpy compares against, staging onto a
device (here: the CPU device) and the binding of a context to torch's current stream, driven with a stand-in context.  No GPU."""

import warnings

import numpy as np
import pytest


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as g

    g.build()
    from pyimcom_amd import _dev

    return _dev


def test_is_torch(dev):
    import torch

    assert dev.is_torch(torch.zeros(2)) is True
    for a in (None, np.zeros(2), [1.0, 2.0]):
        assert dev.is_torch(a) is False


@pytest.mark.parametrize("name", ["float32", "float64", "uint8", "int16", "int32", "int64", "bool", "uint16"])
def test_dtypes_round_trip(dev, name):
    import torch

    assert hasattr(torch, "uint16")  # the code maps are uint16: the installed torch has the type
    td = dev.torch_dtype(np.dtype(name))
    assert td is getattr(torch, name) and dev.torch_dtype(name) is td
    assert dev.np_dtype(torch.zeros(3, dtype=td)) == np.dtype(name)
    assert dev.np_dtype(np.zeros(3, dtype=name)) == np.dtype(name)
    assert dev.torch_dtype(dev.np_dtype(torch.zeros(1, dtype=td))) is td


def test_compare_value(dev):
    cv = dev.compare_value
    x = 0.1234567890123
    assert cv(x, np.float32) == float(np.float32(x)) != x
    assert cv(np.float64(0.7), np.float32) == 0.7
    assert cv(np.float32(0.7), np.float64) == float(np.float32(0.7))  # float32 -> float64 is exact
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert cv(1e300, np.float32) == np.inf
        assert np.isnan(cv(np.nan, np.float32)) and np.isnan(cv(np.float32(np.nan), np.float64))
    assert cv(0.7, np.float32) == float(np.float32(0.7)) and cv(np.float64(0.7), np.float32) == 0.7  # (tests/test_crmask_host.py's pair)
    from pyimcom_amd import objmask

    assert objmask.compare_value is cv


def test_one_default_device(dev):
    from pyimcom_amd import healpix, i24, inpool, metamosaic, objmask, reportstats, starcat, wcs

    assert dev.DEVICE == "cuda:0"
    assert all(m.DEVICE is dev.DEVICE for m in (healpix, i24, inpool, metamosaic, objmask, reportstats, starcat, wcs))


def test_staging(dev):
    import torch

    cpu = torch.device("cpu")
    big = np.arange(12, dtype=">f4").reshape(3, 4)
    t = dev.staged(big, cpu, (np.float32, np.float64), "seam: float32 or float64, not {dtype}")
    assert t.dtype == torch.float32 and np.array_equal(t.numpy(), big) and t.numpy().dtype.isnative
    a = np.arange(24, dtype=np.float64).reshape(4, 6)
    for src in (np.asfortranarray(a), a[:, ::2], torch.as_tensor(a).t().contiguous().t(), torch.as_tensor(a)[:, ::2]):
        t = dev.staged(src, cpu)
        assert t.is_contiguous() and np.array_equal(t.numpy(), np.asarray(src))
    rows = torch.as_tensor(a)[::2, 1:5]  # rows two apart, a crop of each: unit stride along the rows
    assert not rows.is_contiguous()
    t = dev.staged(rows, cpu, layout="rows")
    assert t.data_ptr() == rows.data_ptr() and t.stride() == rows.stride()
    assert dev.staged(rows, cpu).is_contiguous() and dev.staged(rows, cpu).data_ptr() != rows.data_ptr()
    cols = torch.as_tensor(a)[:, ::2]
    assert dev.staged(cols, cpu, layout="rows").is_contiguous() and dev.staged(cols, cpu, layout="any").stride() == cols.stride()
    for bad in (np.zeros(3, dtype=np.int32), torch.zeros(3, dtype=torch.int32)):
        with pytest.raises(TypeError, match="seam XYZ: a float image") as e:
            dev.staged(bad, cpu, (np.float32, np.float64), "seam XYZ: a float image, not {dtype}")
        assert str(e.value).endswith(str(bad.dtype))
    with pytest.raises(TypeError, match="seam XYZ: a float image, not torch.bfloat16"):  # (a torch dtype that numpy has no name for)
        dev.staged(torch.zeros(3, dtype=torch.bfloat16), cpu, (np.float32, np.float64), "seam XYZ: a float image, not {dtype}")
    with pytest.raises(TypeError, match="codes of dtype int32"):
        dev.staged(torch.zeros(3, dtype=torch.int32), cpu, ("uint8", "uint16"), "codes of dtype {name}")
    ok = torch.zeros((3, 4), dtype=torch.float32)
    assert dev.staged(ok, cpu, (np.float32,), "x {dtype}") is ok and dev.staged(ok, cpu, layout="rows") is ok and dev.staged(ok, cpu, astype=np.float32) is ok
    u16 = dev.staged(np.array([0, 1, 65535], dtype=">u2"), cpu)
    assert u16.dtype == torch.uint16 and np.array_equal(u16.numpy(), [0, 1, 65535])
    f = dev.staged(np.array([1, 2, 3], dtype=">i2"), cpu, astype=np.float64)
    assert f.dtype == torch.float64 and f.tolist() == [1.0, 2.0, 3.0]
    assert dev.staged(torch.tensor([1, 2], dtype=torch.int16), cpu, astype=np.float32).dtype == torch.float32
    h = dev.to_host(ok)
    assert isinstance(h, np.ndarray) and h.shape == (3, 4) and dev.to_host(big) is big and isinstance(dev.to_host([1, 2]), np.ndarray)


class _Context:
    device = 1

    def __init__(self):
        self.streams = []

    def set_stream(self, handle):
        self.streams.append(handle)


@pytest.mark.parametrize("form", ["string", "device", "none", "other device"])
def test_binding_takes_the_stream_of_the_contexts_own_device(dev, form, monkeypatch):
    import torch

    asked = []

    def current_stream(device=None):
        asked.append(device)
        return type("Stream", (), {"cuda_stream": 0xBEEF})()

    def names_cuda_1(d):  # (torch.cuda.current_stream takes an index, a string or a torch.device)
        return d == 1 if isinstance(d, int) else torch.device(d) == torch.device("cuda", 1)

    monkeypatch.setattr(torch.cuda, "current_stream", current_stream)
    ctx = _Context()
    arg = {"string": "cuda:1", "device": torch.device("cuda", 1), "none": None, "other device": torch.device("cuda", 0)}[form]
    assert dev.bound_context(arg, ctx) is ctx
    assert ctx.streams == [0xBEEF]
    assert len(asked) == 1 and names_cuda_1(asked[0])
    assert dev.bound_context(ctx=ctx) is ctx and ctx.streams == [0xBEEF] * 2 and names_cuda_1(asked[1])


def test_device_of(dev):
    import torch

    assert dev.device_of(None, np.zeros(2), torch.zeros(2)) == torch.device("cuda:0")  # (a tensor on the host names no device)
    assert dev.device_of(np.zeros(2), device="cuda:3") == torch.device("cuda:3")
