"""``CplxNoise.noise_1f_frame`` (reference src/pyimcom/layer.py:871-913) restated with the length, the number of channels, the channel width
and the border as parameters and the draws as an input, in float64 with numpy's own statements (``restated``: equal to the reference bit for
bit, tests/test_noise1f_host.py) and in extended precision (``np.longdouble``, numpy's transform included) as the yardstick of the device's
float64 transform; and the statement the float32 frames are held to."""

import numpy as np


def amp_of(length):
    """layer.py:892-895."""
    freq = np.linspace(0, 1 - 1.0 / length, length)
    freq[length // 2 :] -= 1.0
    amp = (1.0e-99 + np.abs(freq * length)) ** (-0.5)
    amp[0] = 0.0
    return amp


def draws(seed, length, nch):
    """The draws of layer.py:899-900 for all channels, [2 nch, length]: row 2c the real, row 2c + 1 the imaginary part of channel c."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.normal(loc=0.0, scale=1.0, size=(length,)) for _ in range(2 * nch)])


def restated(normals, amp, w, border=4, extended=False):
    """(blocks [nch, length / 2] after the mean is subtracted, float64 or longdouble; the float32 frame without its border)."""
    nch, length = normals.shape[0] // 2, normals.shape[1]
    rows = length // 2 // w
    ft, ct = (np.longdouble, np.clongdouble) if extended else (np.float64, np.complex128)
    this_array = np.zeros((rows, nch * w), dtype=np.float32)
    blocks = np.zeros((nch, length // 2), dtype=ft)
    for ch in range(nch):
        ftsignal = np.zeros((length,), dtype=ct)
        ftsignal[:] = normals[2 * ch]
        ftsignal[:] += 1j * normals[2 * ch + 1].astype(ft)
        ftsignal *= amp.astype(ft)
        block = np.fft.fft(ftsignal).real[: length // 2] / np.sqrt(ft(2.0))
        block -= np.mean(block)
        blocks[ch] = block
        xmin = ch * w
        xmax = xmin + w
        if ch % 2 == 0:
            this_array[:, xmin:xmax] = block.reshape((rows, w))
        else:
            this_array[:, xmin:xmax] = block.reshape((rows, w))[:, ::-1]
    return blocks, this_array[border : rows - border, border : nch * w - border]


def bound(f64_err, ext_max, floor=2e-13):
    """The bound of the float64 device transform against the extended evaluation: ten times the distance of the float64 numpy run from it,
    with a floor relative to the largest value (another factorisation of the same float64 sums)."""
    return max(10.0 * float(f64_err), floor * float(ext_max))


def straddles(a32, b32):
    """(elements where two float32 roundings of nearly equal values differ, whether every difference is one unit in the last place)."""
    a32, b32 = np.asarray(a32, dtype=np.float32), np.asarray(b32, dtype=np.float32)
    diff = a32 != b32
    one_ulp = np.all((np.nextafter(a32[diff], b32[diff]) == b32[diff]))
    return int(np.count_nonzero(diff)), bool(one_ulp)


def cap(count_f64, n, factor=10):
    """The largest number of elements out of n that may differ: ten times what the float64 numpy run shows against the extended evaluation
    on the same inputs, and one element at least."""
    return max(factor * int(count_f64), 1)
