"""The 1/f noise layer on the device (csrc/noise1f.hip, pyimcom_amd.noiselayers.noise_1f / noise_1f_frame).

The float64 channels before the cast are held to ``max(10 |float64 numpy run - ext|, 2e-13 max |ext|)`` (largest deviations; ext: the
``np.longdouble`` evaluation of tests/noise1f_reference.py on the same draws).  The float32 frame may differ from numpy's only by one unit
in the last place (the two float64 values lie on either side of a float32 rounding boundary), in at most ten times as many pixels as the
float64 numpy run itself differs from the extended evaluation, one pixel at least.  Every test prints its figures (``-s``)."""

import os

import numpy as np
import pytest

from tests import noise1f_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "noise.npz")


def _device(normals, amp, nch, w, border=4):
    import torch

    from pyimcom_amd import noiselayers as nl

    frame, block = nl.noise_1f(torch.from_numpy(normals).to(DEV), amp, nch, w, border=border, return_block=True)
    return frame.cpu().numpy(), block.cpu().numpy()


# len = 2^12 = 64 x 64 with nch = 4, w = 16; 2^10 = 32 x 32, the shortest length the two steps take (a line has 32 points at least); 2^11 =
# 64 x 32, the two steps of different lengths
@pytest.mark.parametrize("length,nch,w", [(1 << 12, 4, 16), (1 << 10, 3, 8), (1 << 11, 2, 32)])
def test_small_frames_against_numpy_and_the_extended_evaluation(length, nch, w):
    from pyimcom_amd import noiselayers as nl

    normals, amp = ref.draws(20261 + length, length, nch), ref.amp_of(length)
    assert amp.tobytes() == nl.noise_1f_amp(length).tobytes()
    b64, f64 = ref.restated(normals, amp, w)
    bext, fext = ref.restated(normals, amp, w, extended=True)
    frame, block = _device(normals, amp, nch, w)
    assert frame.dtype == np.float32 and frame.shape == f64.shape == (length // 2 // w - 8, nch * w - 8) and block.shape == b64.shape
    err64, ext_max = np.abs(b64 - bext).max(), np.abs(bext).max()
    err = np.abs(block - bext).max()
    n64, _ = ref.straddles(f64, fext)
    n_dev, one_ulp = ref.straddles(frame, f64)
    print(f"\nlen {length} nch {nch} w {w}: |device - ext| {float(err):.3e}  |numpy - ext| {float(err64):.3e}  max |ext| {float(ext_max):.3f}  "
          f"float32 pixels that differ: device/numpy {n_dev}, numpy/ext {n64}, of {frame.size}")
    assert err <= ref.bound(err64, ext_max)
    assert one_ulp and n_dev <= ref.cap(n64, frame.size)
    # the same bits again, and through host memory
    frame2, block2 = _device(normals, amp, nch, w)
    assert frame2.tobytes() == frame.tobytes() and block2.tobytes() == block.tobytes()


def test_channel_layout_reversal_and_crop():
    """Draws whose transform is a chosen pattern (the inverse DFT of it, amp = 1): channel c holds 64 c + column + row / 1024, so every pixel
    names its channel, its column inside the channel and its row.  The frame is checked against that pattern indexed directly."""
    length, nch, w, border = 1 << 11, 5, 16, 3
    half, rows = length // 2, length // 2 // w
    i = np.arange(half)
    normals = np.zeros((2 * nch, length))
    pattern = np.zeros((nch, half))
    for c in range(nch):
        pattern[c] = 64 * c + (i % w) + (i // w) / 1024.0
        spectrum = np.zeros(length, dtype=complex)
        spectrum[:half] = pattern[c] * np.sqrt(2.0)
        x = np.fft.ifft(spectrum)
        normals[2 * c], normals[2 * c + 1] = x.real, x.imag
    frame, block = _device(normals, np.ones(length), nch, w, border=border)
    assert frame.shape == (rows - 2 * border, nch * w - 2 * border)
    want = np.zeros((rows, nch * w))
    for c in range(nch):
        for y in range(rows):
            for x in range(w):
                want[y, c * w + (w - 1 - x if c % 2 else x)] = pattern[c, y * w + x] - pattern[c].mean()
    want = want[border : rows - border, border : nch * w - border]
    print("\nlargest deviation from the pattern", np.abs(frame - want).max())
    assert np.abs(frame - want).max() < 1e-4  # (a float32 near 320 is within 1.6e-5; the pattern's steps are 1 and 1 / 1024)
    assert np.abs(block - (pattern - pattern.mean(axis=1, keepdims=True))).max() < 1e-9


def test_sides_that_are_no_powers_of_two_are_unsupported():
    import torch

    from pyimcom_amd import _lib
    from pyimcom_amd import noiselayers as nl

    for length, nch, w in [(3000, 2, 8), (1 << 9, 2, 8), (1 << 21, 1, 8), (1 << 12, 2, 24), (1 << 10, 1, 1 << 10)]:
        g = torch.zeros((2 * nch, length), dtype=torch.float64, device=DEV)
        with pytest.raises(_lib.ImcomError) as e:
            nl.noise_1f(g, np.ones(length), nch, w, border=0)
        assert e.value.status == -4, (length, w, e.value)  # IMCOM_ERR_UNSUPPORTED
    g = torch.zeros((4, 1 << 10), dtype=torch.float64, device=DEV)
    with pytest.raises(_lib.ImcomError) as e:  # a border that leaves nothing of 64 x 16 pixels
        nl.noise_1f(g, np.ones(1 << 10), 2, 8, border=8)
    assert e.value.status == -1  # IMCOM_ERR_ARG


def test_full_frame_against_the_golden():
    """One ``noise_1f_frame(seed)`` at the production size against the rows, columns, slice and channel sums of the reference's own run."""
    from pyimcom_amd import noiselayers as nl

    g = np.load(GOLDEN)
    frame = nl.noise_1f_frame(int(g["f1_seed"]))
    assert frame.dtype == np.float32 and frame.shape == (4088, 4088)
    assert nl.last_info["undecided"] == 0
    lines = g["lines"]
    r0, r1, c0, c1 = g["slice"]
    n_r, ok_r = ref.straddles(frame[lines, :], g["f1_rows"])
    n_c, ok_c = ref.straddles(frame[:, lines], g["f1_cols"])
    n_s, ok_s = ref.straddles(frame[r0:r1, c0:c1], g["f1_slice"])
    allowed = ref.cap(int(g["f1_f64_straddles"]), 2 * lines.size * 4088)
    print(f"\nfloat32 pixels that differ from the reference's: rows {n_r}, columns {n_c}, slice {n_s}; the reference's float64 run against the "
          f"extended evaluation on the same rows and columns: {int(g['f1_f64_straddles'])} (whole frame: {int(g['f1_f64_straddles_frame'])})")
    assert ok_r and ok_c and ok_s and n_r + n_c <= allowed and n_s <= 1
    # a channel's sum moves by one float32 unit in the last place per pixel that differs: ten times the reference's own count over the
    # frame (one at least), each worth at most the spacing of float32 at the frame's largest value
    edges = [0, 124] + [128 * c - 4 for c in range(2, 32)] + [4088]
    sums = np.array([frame[:, a:b].sum(dtype=np.float64) for a, b in zip(edges[:-1], edges[1:])])
    tol = ref.cap(int(g["f1_f64_straddles_frame"]), frame.size) * float(np.spacing(np.float32(np.abs(frame).max())))
    print("channel sums: largest deviation", np.abs(sums - g["f1_ch_sum"]).max(), "allowed", tol)
    assert np.abs(sums - g["f1_ch_sum"]).max() <= tol


def test_float64_channels_at_the_production_size():
    """The 1024 x 1024 split in float64: the channels of one production frame before the cast.  Channels 0 and 31 (the first, and the last
    of the fourth group of eight, a reversed one) are held to the float64 bound against the extended evaluation of the same draws, which
    are copied from the device; every channel's mean is zero to a few roundings of its largest value."""
    import torch

    from pyimcom_amd import noiselayers as nl

    length, nch, w = 8192 * 128, 32, 128
    g = np.load(GOLDEN)
    normals = nl.standard_normal(np.random.PCG64(int(g["f1_seed"])), (2 * nch, length), device=DEV)
    amp = ref.amp_of(length)
    frame, block = nl.noise_1f(normals, amp, nch, w, return_block=True)
    block = block.cpu().numpy()
    assert frame.shape == (4088, 4088) and block.shape == (nch, length // 2)
    means = np.abs(block.mean(axis=1))
    print(f"\nlargest |channel mean| {means.max():.3e} at max |block| {np.abs(block).max():.3f}")
    assert means.max() <= 8 * np.finfo(np.float64).eps * np.abs(block).max()  # (the mean subtracted and the mean taken here: two float64 sums)
    for ch in (0, 31):
        pair = normals[2 * ch : 2 * ch + 2].cpu().numpy()
        b64, _ = ref.restated(pair, amp, w)
        bext, _ = ref.restated(pair, amp, w, extended=True)
        err64, ext_max, err = np.abs(b64 - bext).max(), np.abs(bext).max(), np.abs(block[ch] - bext[0]).max()
        print(f"channel {ch}: |device - ext| {float(err):.3e}  |numpy - ext| {float(err64):.3e}  max |ext| {float(ext_max):.3f}")
        assert err <= ref.bound(err64, ext_max)
        want = np.float32(b64[0]).reshape(4096, w)[:, ::-1 if ch % 2 else 1][4:4092]
        got = frame[:, max(ch * w - 4, 0) : ch * w - 4 + w].cpu().numpy()
        n, one_ulp = ref.straddles(got, want[:, 4:] if ch == 0 else want[:, : got.shape[1]])
        assert one_ulp and n <= 1


def test_device_output_of_the_frame():
    import torch

    from pyimcom_amd import noiselayers as nl

    a = nl.noise_1f_frame(5, device_out=True, _length=1 << 12, _nch=4, _w=16)
    b = nl.noise_1f_frame(5, _length=1 << 12, _nch=4, _w=16)
    assert isinstance(a, torch.Tensor) and a.is_cuda and isinstance(b, np.ndarray) and a.cpu().numpy().tobytes() == b.tobytes()
    _, f64 = ref.restated(ref.draws(5, 1 << 12, 4), ref.amp_of(1 << 12), 16)
    n, one_ulp = ref.straddles(b, f64)
    assert one_ulp and n <= 1
