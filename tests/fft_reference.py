"""Test infrastructure: what the wave-per-line FFT engine (pyimcom_amd/csrc/fft_lines.h, fft_plan_core.h, fft.hip and the line kernels of
psf_overlap.hip) computes behind imcom_psf_spectra and imcom_psf_overlap_spectra, restated with numpy and scipy in the buffers' own
layouts, in float64 (numpy.fft) and in extended precision (``extended=True``: scipy.fft on numpy.longdouble / numpy.clongdouble, the
yardstick convention of tests/splitpsf_reference.py).  tests/test_fft_reference.py pins it to numpy's rfft2 / irfft2 and to the oracle.
Not part of the package, and it imports nothing from it."""

import numpy as np
import scipy.fft

EPS64 = float(np.finfo(np.float64).eps)
HAVE_EXTENDED = bool(np.finfo(np.longdouble).eps < 1e-18)  # the 80-bit type (eps 1.08e-19); the GPU tests skip without it
BORDER = 6  # zero samples around a table (the interpolators' reach)


def plan_sides():
    """The sides the butterflies take: 6 <= n <= 1024, a product of 16, 8, 4, 2, 3, 5 taken greedily in that order, at least two factors
    (so 4, 8 and 16 -- one radix each -- are none).  The waves and the LDS never rule a side out below 1024 (tests/test_fft_plan.py)."""
    sides = []
    for n in range(6, 1025):
        r, nst = n, 0
        for c in (16, 8, 4, 2, 3, 5):
            while r % c == 0:
                r //= c
                nst += 1
        if r == 1 and nst >= 2:
            sides.append(n)
    return sides


def _real(extended):
    assert not extended or HAVE_EXTENDED, "numpy.longdouble is no wider than float64 here: no yardstick"
    return np.longdouble if extended else np.float64


def spectra(psfs, nfft, extended=False):
    """[p][kx < nfft/2+1][ky < nfft] complex: the rfft2 of every PSF [p][y][x] zero-padded into the corner of an nfft x nfft frame, in the
    layout of the resident buffer -- numpy's [ky][kx] transposed."""
    psfs = np.asarray(psfs, dtype=np.float64)
    npsf, ns, _ = psfs.shape
    assert ns <= nfft and nfft % 2 == 0
    frame = np.zeros((npsf, nfft, nfft), dtype=_real(extended))
    frame[:, :ns, :ns] = psfs
    r = scipy.fft.rfft2(frame, axes=(1, 2)) if extended else np.fft.rfft2(frame, axes=(1, 2))
    return np.ascontiguousarray(np.swapaxes(r, 1, 2))


def mode_weight(nfft, amp):
    """[kx][ky]: 1 + a0 exp(-2 pi^2 |u|^2 a1^2), u = k / nfft wrapped to (-1/2, 1/2] (float64: part of the input, not of the transform)."""
    a0, a1 = float(amp[0]), float(amp[1])
    ux = np.arange(nfft // 2 + 1) / nfft
    uy = np.arange(nfft) / nfft
    ux, uy = np.where(ux > 0.5, ux - 1.0, ux), np.where(uy > 0.5, uy - 1.0, uy)
    return 1.0 + a0 * np.exp(-2.0 * np.pi**2 * (ux[:, None] ** 2 + uy[None, :] ** 2) * a1**2)


def product(s1, s2, nfft, amp=None):
    """spec1 conj(spec2) w^2 of one pair, [kx][ky], in the precision of its operands."""
    z = s1 * np.conj(s2)
    if amp is not None:
        w = mode_weight(nfft, amp)
        z = z * (w * w).astype(z.real.dtype)
    return z


def inverse(z, nfft, extended=False):
    """[y][x] real, nfft x nfft, from the half spectrum z [kx][ky] the way the kernels state it: a complex inverse along ky for every kx
    column, then a complex-to-real inverse along kx that takes only the real parts of the columns kx = 0 and kx = nfft / 2 (numpy's c2r
    does the same).  So a spectrum that is not Hermitian-consistent has a defined answer."""
    nh = nfft // 2 + 1
    assert z.shape == (nh, nfft)
    z = z.astype(np.clongdouble if extended else np.complex128)
    fft = scipy.fft if extended else np.fft
    v = fft.ifft(z, axis=1)  # [kx][y]
    v[0] = v[0].real
    v[nh - 1] = v[nh - 1].real
    return np.ascontiguousarray(fft.irfft(v, n=nfft, axis=0).T)  # [x][y] -> [y][x]


def tables(spec1, spec2, pairs, ntab, nfft, extended=False, amp=None):
    """[pair][ntab + 12][ntab + 12]: for every pair (p, q) the inverse of spec1[p] conj(spec2[q]) w^2, rolled by ntab // 2 along both axes,
    cropped to ntab x ntab, inside the 6-sample zero border."""
    assert 1 <= ntab <= nfft - 1
    cdt = np.clongdouble if extended else np.complex128
    spec1, spec2 = np.asarray(spec1).astype(cdt), np.asarray(spec2).astype(cdt)
    nc, ng = ntab // 2, ntab + 2 * BORDER
    out = np.zeros((len(pairs), ng, ng), dtype=_real(extended))
    for t, (p, q) in enumerate(pairs):
        full = inverse(product(spec1[p], spec2[q], nfft, amp), nfft, extended)
        out[t, BORDER:-BORDER, BORDER:-BORDER] = np.roll(full, (nc, nc), axis=(0, 1))[:ntab, :ntab]
    return out


def yardstick(a64, aext):
    """max |float64 numpy result - extended result|: the reference's own rounding on this input."""
    return float(np.abs(np.asarray(a64).astype(np.clongdouble if np.iscomplexobj(a64) else np.longdouble) - aext).max())


def norm2(a):
    return float(np.sqrt(np.sum(np.abs(np.asarray(a)) ** 2)))


def bound(yard, n2, factor=10.0):
    """The distance per bin the device may have from the extended-precision result: ten times the larger of the float64 reference's own
    distance and eps64 ||input||_2 (the floor keeps the bound meaningful at the tiny sides where numpy happens to be exact).  factor = 11
    where the device is compared with the float64 reference instead (the triangle inequality)."""
    return factor * max(float(yard), EPS64 * float(n2))
