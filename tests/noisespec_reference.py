"""A numpy restatement of the noise power spectra (reference src/pyimcom/analysis.py:661-807, 1253-1303 and
src/pyimcom/diagnostics/noise_diagnostics.py:400-506) in float64, for sides too large to commit as golden vectors, with an extended-precision
evaluation (``extended=True``: scipy.fft on numpy.longdouble, sums in longdouble) -- the yardstick of a float64 path's own rounding."""

import numpy as np
import scipy.fft


def fold_rfft2(frame, norm):
    """analysis.py:789-793 as written: the shifted full spectrum folded out of rfft2 (in the precision numpy gives the input)."""
    Lcut = frame.shape[0]
    ps = np.empty((Lcut, Lcut), dtype=np.float64)
    rps = np.square(np.abs(np.fft.fftshift(np.fft.rfft2(frame), 0))) / norm
    ps[:, Lcut // 2:] = rps[:, :-1]
    ps[1:, : Lcut // 2] = rps[Lcut - 1: 0: -1, Lcut // 2: 0: -1]
    ps[0, : Lcut // 2] = rps[0, Lcut // 2: 0: -1]
    return ps


def power_spectrum_2d(frame, norm=1.0, window=None, bin8=True, extended=False):
    """fftshift(|fft2(frame * window)|^2) / norm, averaged over 8 x 8 cells with bin8 (analysis.py:789-794, noise_diagnostics.py:430-441)."""
    ft = np.longdouble if extended else np.float64
    a = np.asarray(frame).astype(ft)
    if window is not None:
        a = a * np.asarray(window).astype(ft)
    F = scipy.fft.fft2(a.astype(np.clongdouble)) if extended else np.fft.fft2(a)
    ps = np.fft.fftshift(F.real**2 + F.imag**2) / ft(norm)
    if bin8:
        L = ps.shape[0]
        ps = np.average(np.reshape(ps, (L // 8, 8, L // 8, 8)), axis=(1, 3))
    return ps


def radial_labels(n, nradbins):
    """analysis.py:691-695."""
    yy, xx = np.mgrid[:n, :n]
    r = np.hypot(xx - n / 2, yy - n / 2)
    return (nradbins * r / r.max()).astype(int)


def azimuthal_average(image, nradbins, rbin=None, extended=False):
    """analysis.py:691-702: (mean, err) over the labels 1 .. rbin.max(), err = sqrt(mean((x - mean)^2)) / sqrt(npix)."""
    ft = np.longdouble if extended else np.float64
    image = np.asarray(image).astype(ft)
    if rbin is None:
        rbin = radial_labels(image.shape[0], nradbins)
    nidx = int(rbin.max())
    mean, err = np.full(nidx, np.nan, dtype=ft), np.full(nidx, np.nan, dtype=ft)
    for i in range(1, nidx + 1):
        v = image[rbin == i]
        if v.size:
            mean[i - 1] = v.sum() / v.size
            err[i - 1] = np.sqrt(((v - mean[i - 1]) ** 2).sum() / v.size) / np.sqrt(ft(v.size))
    return mean, err


def wavenumbers(L, nradbins):
    """analysis.py:735-740."""
    k = np.fft.fftshift(np.fft.fftfreq(L))
    kx, ky = np.meshgrid(k, k)
    return azimuthal_average(np.sqrt(np.square(kx) + np.square(ky)), nradbins)[0]


def noise_anal(indata, bdpad, norm_of, extended=False):
    """NoiseAnal.__call__ (analysis.py:776-807) for a block array: crop by bdpad, then to Lcut; norm_of(Lcut) -> norm.  (ps2d, ps1d)."""
    if bdpad:
        indata = indata[bdpad:-bdpad, bdpad:-bdpad]
    Lcut = indata.shape[0] // 8 * 8
    ps2d = power_spectrum_2d(indata[:Lcut, :Lcut], norm_of(Lcut), None, True, extended)
    mean, err = azimuthal_average(ps2d, Lcut // 16, None, extended)
    return ps2d, np.stack((mean, err), axis=1)


def mosaic(blocks, coverage_idx, bins, norm):
    """analysis.py:1253-1303 for blocks [nby][nbx][nlayer, L, L] and coverage_idx [nby][nbx]: (ps2d_all, ps1d_all)."""
    nblock, nlayer, L = len(blocks), blocks[0][0].shape[0], blocks[0][0].shape[-1]
    coverage_idx = np.asarray(coverage_idx)
    unique, counts = np.unique(coverage_idx, return_counts=True)
    ps2d_all = np.zeros((nlayer, L // 8, L // 8))
    ps1d_all = np.zeros((nlayer, bins, L // 16, 2))
    rbin = radial_labels(L // 8, L // 16)
    for iby in range(nblock):
        for inl in range(nlayer):
            for ibx in range(nblock):
                ps2d = power_spectrum_2d(blocks[iby][ibx][inl], norm)
                mean, err = azimuthal_average(ps2d, L // 16, rbin)
                ps2d_all[inl] += ps2d
                ps1d_all[inl, coverage_idx[iby][ibx], :, 0] += mean
                ps1d_all[inl, coverage_idx[iby][ibx], :, 1] += err
    ps2d_all /= nblock**2
    for idx, count in zip(unique, counts):
        ps1d_all[:, idx, :, :] /= count
    return ps2d_all, ps1d_all


def bound(f64_err, ext_max, floor=2e-13):
    """The bound of a float64 device path against the extended evaluation: ten times the distance of the float64 numpy run from it, with a
    floor relative to the largest value (another summation order of the same float64 arithmetic)."""
    return max(10.0 * float(f64_err), floor * float(ext_max))
