"""tests/fft_reference.py is the yardstick of tests/test_gpu_fft_edges.py; here its float64 form is pinned to numpy's own rfft2 / irfft2 and
to the oracle, its layout to impulses, its list of sides to the facts tests/test_fft_plan.py pins, and its extended form to the float64
one, so that the GPU tests cannot be wrong in their reference."""

import numpy as np
import pytest

from tests import fft_reference as fr


def _psfs(rng, n, ns):
    p = rng.standard_normal((n, ns, ns))
    p[:, -1, -1] += 1.0
    return p


def _frames(p, nfft):
    f = np.zeros((p.shape[0], nfft, nfft))
    f[:, : p.shape[1], : p.shape[2]] = p
    return f


@pytest.mark.parametrize("nfft,ns", [(6, 3), (60, 29), (512, 255), (512, 1)])
def test_spectra_is_numpys_rfft2_transposed(nfft, ns):
    p = _psfs(np.random.default_rng(nfft + ns), 2, ns)
    got = fr.spectra(p, nfft)
    want = np.fft.rfft2(_frames(p, nfft)).transpose(0, 2, 1)
    assert got.shape == (2, nfft // 2 + 1, nfft) and got.dtype == np.complex128 and got.flags.c_contiguous
    assert np.array_equal(got, want)


def test_layout_by_impulses():
    """An impulse at (y, x) = (1, 0) varies along ky only, one at (0, 1) along kx only: buffer[p][kx][ky]."""
    nfft = 12
    p = np.zeros((2, 5, 5))
    p[0, 1, 0] = 1.0
    p[1, 0, 1] = 1.0
    s = fr.spectra(p, nfft)
    kx, ky = np.arange(nfft // 2 + 1)[:, None], np.arange(nfft)[None, :]
    np.testing.assert_allclose(s[0], np.exp(-2j * np.pi * ky / nfft) + 0 * kx, rtol=0, atol=1e-14)
    np.testing.assert_allclose(s[1], np.exp(-2j * np.pi * kx / nfft) + 0 * ky, rtol=0, atol=1e-14)
    # and back: the table holds the PSF's cyclic correlation with an impulse at the origin, rolled by ntab // 2
    one = fr.spectra(np.ones((1, 1, 1)), nfft)
    assert np.array_equal(one, np.ones((1, nfft // 2 + 1, nfft)))
    t = fr.tables(s, one, [(0, 0), (1, 0)], 5, nfft)
    want = np.zeros((2, 17, 17))
    want[0, 6 + 2 + 1, 6 + 2] = 1.0
    want[1, 6 + 2, 6 + 2 + 1] = 1.0
    np.testing.assert_allclose(t, want, rtol=0, atol=1e-14)


@pytest.mark.parametrize("nfft,ns,ntab", [(6, 3, 3), (60, 29, 29), (80, 33, 79), (512, 255, 255)])
def test_tables_is_numpys_irfft2_rolled_and_cropped(nfft, ns, ntab):
    rng = np.random.default_rng(nfft)
    s1, s2 = fr.spectra(_psfs(rng, 2, ns), nfft), fr.spectra(_psfs(rng, 2, ns), nfft)
    pairs = [(0, 1), (1, 0), (1, 1)]
    for amp in (None, (0.3, 1.8)):
        got = fr.tables(s1, s2, pairs, ntab, nfft, amp=amp)
        assert got.shape == (3, ntab + 12, ntab + 12) and got.dtype == np.float64
        uy, ux = np.fft.fftfreq(nfft)[:, None], np.fft.rfftfreq(nfft)[None, :]  # numpy's [ky][kx]; rfftfreq's Nyquist is +1/2 as in the kernel
        w = 1.0 if amp is None else 1.0 + amp[0] * np.exp(-2.0 * np.pi**2 * (ux**2 + uy**2) * amp[1] ** 2)
        for t, (p, q) in enumerate(pairs):
            z = s1[p].T * np.conj(s2[q].T) * w * w
            want = np.roll(np.fft.irfft2(z, s=(nfft, nfft)), (ntab // 2, ntab // 2), axis=(0, 1))[:ntab, :ntab]
            scale = np.abs(want).max()
            assert np.abs(got[t, 6:-6, 6:-6] - want).max() <= 1e-14 * scale, (nfft, amp, t)
        border = got.copy()
        border[:, 6:-6, 6:-6] = 0.0
        assert np.all(border == 0.0)


@pytest.mark.parametrize("nfft", [6, 60, 512])
def test_non_hermitian_input_has_numpys_answer(nfft):
    """O(1) real and imaginary parts in every bin, DC and Nyquist rows and columns included: a complex inverse along ky, then numpy's
    c2r along kx, which ignores the imaginary parts of the columns 0 and nfft / 2."""
    rng = np.random.default_rng(nfft)
    nh = nfft // 2 + 1
    z = rng.standard_normal((nh, nfft)) + 1j * rng.standard_normal((nh, nfft))
    got = fr.inverse(z, nfft)
    want = np.fft.irfft(np.fft.ifft(z, axis=1), n=nfft, axis=0).T
    assert got.shape == (nfft, nfft)
    assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max()
    # numpy's irfft2 takes the same decomposition (c2c along the first axes, c2r along the last)
    want2 = np.fft.irfft2(z.T, s=(nfft, nfft))
    assert np.abs(got - want2).max() <= 1e-14 * np.abs(want2).max()
    # the rule matters on this input: what the c2r drops is as large as what it keeps, and keeping it would change the answer
    v = np.fft.ifft(z, axis=1)
    assert np.abs(v[0].imag).max() > 0.1 * np.abs(v[0].real).max() and np.abs(v[nh - 1].imag).max() > 0.1 * np.abs(v[nh - 1].real).max()
    full = np.concatenate([v, np.conj(v[-2:0:-1])])  # the Hermitian extension with the two columns left complex
    kept = np.fft.ifft(full, axis=0).T
    assert np.abs(kept.imag).max() > 0.01 * np.abs(want).max()
    assert np.abs(kept.real - want).max() <= 1e-14 * np.abs(want).max()


def test_tables_agree_with_the_oracle():
    from oracle import oracle as orc

    geo = orc.Geom(5, 6, 0.04 / 3600.0, 0.0)
    ns, nfft = geo.nsamp, geo.nfft
    assert (ns, nfft) == (29, 60)
    rng = np.random.default_rng(1)
    p1, p2 = _psfs(rng, 3, ns), _psfs(rng, 2, ns)
    r1, r2 = orc.pad_and_rfft2(p1, geo), orc.pad_and_rfft2(p2, geo)  # [p][ky][kx]
    s1, s2 = fr.spectra(p1, nfft), fr.spectra(p2, nfft)
    assert np.abs(s1 - r1.transpose(0, 2, 1)).max() <= 1e-13 * np.abs(r1).max()
    want = orc.overlap_cross(r1, r2, geo)
    pairs = [(i, j) for i in range(3) for j in range(2)]
    got = fr.tables(s1, s2, pairs, ns, nfft)[:, 6:-6, 6:-6].reshape(3, 2, ns, ns)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


def test_plan_sides():
    s = fr.plan_sides()
    assert len(s) == 80 and s == sorted(set(s)) and s[:6] == [6, 9, 10, 12, 15, 18] and s[-1] == 1024
    odd = [n for n in s if n % 2]
    assert odd == [9, 15, 25, 27, 45, 75, 81, 125, 135, 225, 243, 375, 405, 625, 675, 729]
    assert not any(n in s for n in (4, 8, 16)) and all(n in s for n in (512, 768, 1024, 486, 810, 972, 1000))


@pytest.mark.skipif(not fr.HAVE_EXTENDED, reason="numpy.longdouble is no wider than float64 on this platform")
def test_extended_form_and_the_bound():
    """The extended form is the same arithmetic (a few eps64 ||x||_2 from the float64 one, as numpy's FFT error goes, and not zero); the
    bound is ten times the larger of the yardstick and the floor."""
    rng = np.random.default_rng(7)
    nfft, ns = 128, 63
    p = _psfs(rng, 1, ns)
    a, b = fr.spectra(p, nfft), fr.spectra(p, nfft, extended=True)
    assert b.dtype == np.clongdouble
    y = fr.yardstick(a, b)
    assert 0.0 < y <= 10.0 * fr.EPS64 * fr.norm2(p)
    nh = nfft // 2 + 1
    z = rng.standard_normal((1, nh, nfft)) + 1j * rng.standard_normal((1, nh, nfft))
    one = np.ones((1, nh, nfft))
    ta, tb = fr.tables(z, one, [(0, 0)], ns, nfft), fr.tables(z, one, [(0, 0)], ns, nfft, extended=True)
    assert tb.dtype == np.longdouble
    y = fr.yardstick(ta, tb)
    assert 0.0 < y <= 10.0 * fr.EPS64 * fr.norm2(z) / nfft
    assert fr.bound(3.0, 1.0) == 30.0 and fr.bound(0.0, 2.0) == 20.0 * fr.EPS64 and fr.bound(1.0, 0.0, factor=11.0) == 11.0
