"""The wave-per-line FFT engine (csrc/fft_lines.h, fft_plan_core.h, fft.hip, the line kernels of psf_overlap.hip and splitpsf.hip) on the
device, directly and bin by bin, at every side its plan takes: the forward 2-D real transform through imcom_psf_spectra (the resident
spectra buffer [p][kx][ky] itself), the inverse pair through imcom_psf_overlap_spectra with a second spectrum of all ones (the table is
then the rolled, cropped inverse of the first), the complex line transforms at odd sides through imcom_splitpsf_tophat with width 1
(side n + 8, a filter that is >= 0.4 over the whole band), and the dense-DFT fallback of fft.hip at the edges of its padding.

Inputs are broadband: standard-normal samples plus a unit impulse in the last sample; spectra handed to the inverse have O(1) real and
imaginary parts in EVERY bin, the DC and Nyquist rows and columns included, so they are not Hermitian-consistent and the rule "the
imaginary parts of the DC and Nyquist columns do not count, as in numpy's c2r" is part of what is checked.  Every output buffer is
filled with NaN (a sentinel where a refusal must leave it alone) before the call, every element the entry promises must come back finite,
nothing is masked.

Yardstick and bound (tests/fft_reference.py, pinned by tests/test_fft_reference.py): the same transform by scipy.fft on numpy.longdouble;
    |device - extended| <= 10 max(yard, eps64 ||input||_2)   per bin,
yard = max |numpy float64 - extended| on the same input, ||input||_2 the norm of the PSF (forward) or of the spectrum / nfft (inverse);
the factor 10 is the one of tests/test_gpu_splitpsf.py (another factorisation of the transforms, FMA contraction; here also the
two-for-one packing of real rows).  Where every PSF or table of a large set is compared with the float64 reference instead, 11 max(...).
The tophat cases keep the bound of tests/splitpsf_reference.py.  Every test prints the largest ratio
|device - extended| / max(yard, eps64 ||input||_2) it found before it asserts (the bound is ratio <= 10).

Largest ratios measured on an MI355X, per group (RATIOS below): 1.9 for the forward transforms (a, nfft = 54), 1.2 for the short inputs (b),
0.38 and 0.12 for the inverses (c, d: their floor eps64 ||spectrum||_2 / nfft is generous), 1.0 against the extended and 1.5 against the
float64 reference for the persistent loops (e, nfft = 1024); the tophat cases (f) come within 0.005 (lines) and 0.014 (dense, N = 448) of
their bound."""

import ctypes as C

import numpy as np
import pytest

from tests import fft_reference as fr
from tests import splitpsf_reference as spref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not fr.HAVE_EXTENDED, reason="numpy.longdouble is no wider than float64 on this platform")]

# largest ratio |device - extended| / max(yard, eps64 ||input||_2) per group as measured on an MI355X (the bound is 10; 11 for `e all`, where
# the device is compared with the float64 reference); f: |device - extended| over a tenth of the bound of tests/splitpsf_reference.py
RATIOS = {"a": 1.944, "b": 1.201, "c": 0.377, "d": 0.122, "e": 1.033, "e all": 1.471, "f lines": 0.051, "f dense": 0.136}

EVEN = [n for n in fr.plan_sides() if n % 2 == 0]
ODD = [n for n in fr.plan_sides() if n % 2 == 1]
STATIC = (512, 768, 1024)
NAN = float("nan")


def _dev():
    import torch

    from pyimcom_amd._lib import default_context

    ctx = default_context()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    return torch, ctx


def _dp(t):
    return C.c_void_p(t.data_ptr())


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


def _largest_odd_half(nfft):
    return (nfft // 2 - 1) | 1


def _psfs(seed, n, ns):
    p = np.random.default_rng(seed).standard_normal((n, ns, ns))
    p[:, -1, -1] += 1.0
    return p


def _random_spectra(seed, n, nfft):
    rng = np.random.default_rng(seed)
    nh = nfft // 2 + 1
    return rng.standard_normal((n, nh, nfft)) + 1j * rng.standard_normal((n, nh, nfft))


def _forward(psfs, nfft):
    """imcom_psf_spectra on a NaN-filled buffer -> [p][kx][ky] complex128; the size entry is checked on the way."""
    from pyimcom_amd._lib import check, lib

    torch, ctx = _dev()
    n, ns, _ = psfs.shape
    nh = nfft // 2 + 1
    size = int(lib.imcom_psf_spectra_size(ns, nfft))
    assert size == 2 * nh * nfft
    t = torch.as_tensor(np.ascontiguousarray(psfs), device="cuda:0")
    spec = torch.full((n, size), NAN, dtype=torch.float64, device="cuda:0")
    check(lib.imcom_psf_spectra(ctx.handle, _dp(t), n, ns, nfft, _dp(spec)))
    torch.cuda.synchronize()
    got = spec.cpu().numpy().view(np.complex128).reshape(n, nh, nfft)
    assert np.isfinite(got.view(np.float64)).all(), f"{int((~np.isfinite(got.view(np.float64))).sum())} values of the spectra were not written"
    return got


def _inverse(spec1, spec2, pairs, nsamp, nfft, amp=None, ntab=None):
    """imcom_psf_overlap_spectra (ntab None) or imcom_psf_overlap_spectra_wide on NaN-filled tables -> [pair][side + 12][side + 12]; every
    element finite, the border exactly zero."""
    from pyimcom_amd._lib import check, lib

    torch, ctx = _dev()
    s1 = torch.as_tensor(np.ascontiguousarray(spec1, dtype=np.complex128), device="cuda:0")
    s2 = torch.as_tensor(np.ascontiguousarray(spec2, dtype=np.complex128), device="cuda:0")
    pr = np.ascontiguousarray(pairs, dtype=np.int32)
    a = None if amp is None else np.array(amp, dtype=np.float64)
    side = nsamp if ntab is None else ntab
    out = torch.full((len(pr), side + 12, side + 12), NAN, dtype=torch.float64, device="cuda:0")
    if ntab is None:
        check(lib.imcom_psf_overlap_spectra(ctx.handle, _dp(s1), len(spec1), _dp(s2), len(spec2), nsamp, nfft, _hp(pr), len(pr), None if a is None else _hp(a),
                                            _dp(out)))
    else:
        check(lib.imcom_psf_overlap_spectra_wide(ctx.handle, _dp(s1), len(spec1), _dp(s2), len(spec2), nsamp, ntab, nfft, _hp(pr), len(pr),
                                                 None if a is None else _hp(a), None, None, 0, _dp(out)))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isfinite(got).all(), f"{int((~np.isfinite(got)).sum())} table values were not written"
    border = got.copy()
    border[:, 6:-6, 6:-6] = 0.0
    assert np.all(border == 0.0)
    return got


def _ratio(got, ext, yard, n2):
    """max |device - extended| over the bins, in units of max(yard, eps64 ||input||_2)."""
    d = float(np.abs(got - ext).max())
    return d / (fr.bound(yard, n2) / 10.0)


def _report(label, worst, limit=10.0):
    print(f"fft-edges {label}: largest |device - extended| / max(yard, eps64 |input|_2) = {worst:.3f} (bound {limit:g})")
    assert worst <= limit, label


def _forward_against_extended(label, psfs, nfft):
    got = _forward(psfs, nfft)
    f64, ext = fr.spectra(psfs, nfft), fr.spectra(psfs, nfft, extended=True)
    assert got.shape == ext.shape
    worst = max(_ratio(got[p], ext[p], fr.yardstick(f64[p], ext[p]), fr.norm2(psfs[p])) for p in range(len(psfs)))
    _report(label, worst)


# ---- a. forward, every even side -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft", EVEN)
def test_forward_every_even_side(nfft):
    """Two PSFs of the largest odd side <= nfft / 2: the last workgroup of rows and of columns is ragged at every plan's wave count."""
    ns = _largest_odd_half(nfft)
    _forward_against_extended(f"a forward nfft={nfft} nsamp={ns}", _psfs(nfft, 2, ns), nfft)


# ---- b. forward, short inputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft", [6, 60, 486, 512])
@pytest.mark.parametrize("ns", [1, 3])
def test_forward_short_inputs(nfft, ns):
    """One and three rows: the lone last row of the two-for-one packing carries half (all) of the input, every load beyond ns is zero."""
    _forward_against_extended(f"b forward nfft={nfft} nsamp={ns}", _psfs(1000 * ns + nfft, 2, ns), nfft)


# ---- c. inverse, every even side ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft", EVEN)
def test_inverse_every_even_side_on_non_hermitian_spectra(nfft):
    ns = _largest_odd_half(nfft)
    nh = nfft // 2 + 1
    spec1, ones = _random_spectra(nfft, 3, nfft), np.ones((1, nh, nfft), dtype=np.complex128)
    pairs = [(0, 0), (1, 0), (2, 0)]
    got = _inverse(spec1, ones, pairs, ns, nfft)
    f64, ext = fr.tables(spec1, ones, pairs, ns, nfft), fr.tables(spec1, ones, pairs, ns, nfft, extended=True)
    assert got.shape == ext.shape
    worst = max(_ratio(got[t], ext[t], fr.yardstick(f64[t], ext[t]), fr.norm2(spec1[t]) / nfft) for t in range(3))
    _report(f"c inverse nfft={nfft} ntab={ns}", worst)


# ---- d. inverse, product and weights --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft", [60, 80, 512, 768, 960])
def test_inverse_product_order_and_mode_weights(nfft):
    """Two random sets of spectra: the pairs (0, 1) and (1, 0) tell which factor is conjugated and which set an index goes to; with
    amp_penalty the per-bin weight (and the wrap of its frequencies beyond 1/2) shows in every bin of a broadband product.  At 512 also the
    wide table of side nfft - 1, whose roll wraps through every row."""
    ns = _largest_odd_half(nfft)
    spec1, spec2 = _random_spectra(nfft, 2, nfft), _random_spectra(nfft + 1, 2, nfft)
    pairs = [(0, 1), (1, 0)]
    plain = fr.tables(spec1, spec2, pairs, ns, nfft)
    # the test can tell: the other order of the pairs and the conjugate on the other factor give other tables
    for wrong in (fr.tables(spec1, spec2, pairs[::-1], ns, nfft), fr.tables(spec2, spec1, [(q, p) for p, q in pairs], ns, nfft)):
        assert np.abs(wrong - plain).max() > 1e-3 * np.abs(plain).max()
    calls = [(None, None), ((0.3, 1.8), None)] + ([(None, nfft - 1), ((0.3, 1.8), nfft - 1)] if nfft == 512 else [])
    for amp, ntab in calls:
        got = _inverse(spec1, spec2, pairs, ns, nfft, amp=amp, ntab=ntab)
        side = ns if ntab is None else ntab
        f64 = plain if (amp, ntab) == (None, None) else fr.tables(spec1, spec2, pairs, side, nfft, amp=amp)
        ext = fr.tables(spec1, spec2, pairs, side, nfft, extended=True, amp=amp)
        assert got.shape == ext.shape
        n2 = [fr.norm2(fr.product(spec1[p], spec2[q], nfft, amp)) / nfft for p, q in pairs]
        worst = max(_ratio(got[t], ext[t], fr.yardstick(f64[t], ext[t]), n2[t]) for t in range(2))
        _report(f"d inverse nfft={nfft} ntab={side} amp={amp}", worst)


# ---- e. the static 16 x 16 x r kernels: persistent loops and the XCD partition --------------------------------------------------------
def _static_waves(nfft):
    """Lines per workgroup of the static kernels: as many padded lines (17 n / 16 values) as 160 KiB hold beside the stage tables
    (240 + 256 (r - 1) values), 12 at most."""
    r = nfft // 256
    return min(12, (160 * 1024 - 16 * (240 + 256 * (r - 1))) // (16 * 272 * r))


def _cu():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


_FWD, _INV = {}, {}


def _forward_case(nfft):
    """The PSFs, their float64 spectra and the extended spectra of three of them, computed once per side."""
    if nfft not in _FWD:
        ns = nfft // 2 - 1
        rp = (ns + 1) // 2
        npsf = _cu() * 12 // rp + 1  # more row lines than cu x 12: both persistent loops take a second, ragged trip
        second = min(_cu() * _static_waves(nfft) // rp, npsf - 1)  # the PSF the second trip of the row loop starts in
        psfs = _psfs(nfft + 7, npsf, ns)
        pick = sorted({0, second, npsf - 1})
        _FWD[nfft] = (psfs, fr.spectra(psfs, nfft), pick, fr.spectra(psfs[pick], nfft, extended=True))
    return _FWD[nfft]


@pytest.mark.parametrize("generic", [False, True], ids=["static", "generic"])
@pytest.mark.parametrize("nfft", STATIC)
def test_forward_persistent_loops(nfft, generic, monkeypatch):
    """More than cu x 12 row lines and far more column lines: every wave of the static kernels loops, the last trip is ragged.  All PSFs
    against the float64 reference (11 x: the triangle inequality), the first, the last and the first of the second trip against the
    extended one.  generic: the same through the general kernels at their widest plans (IMCOM_FFT_GENERIC is read at every call)."""
    if generic:
        monkeypatch.setenv("IMCOM_FFT_GENERIC", "1")
    else:
        monkeypatch.delenv("IMCOM_FFT_GENERIC", raising=False)
    psfs, f64, pick, ext = _forward_case(nfft)
    assert len(psfs) * ((psfs.shape[1] + 1) // 2) > _cu() * 12
    got = _forward(psfs, nfft)
    yards = [fr.yardstick(f64[p], ext[i]) for i, p in enumerate(pick)]
    worst = max(_ratio(got[p], ext[i], yards[i], fr.norm2(psfs[p])) for i, p in enumerate(pick))
    _report(f"e forward nfft={nfft} npsf={len(psfs)} {'generic' if generic else 'static'} picked {pick}", worst)
    yard = max(yards)
    worst_all = max(float(np.abs(got[p] - f64[p]).max()) / (fr.bound(yard, fr.norm2(psfs[p])) / 10.0) for p in range(len(psfs)))
    _report(f"e forward nfft={nfft} npsf={len(psfs)} {'generic' if generic else 'static'} all against float64", worst_all, 11.0)


def _inverse_case(nfft):
    if nfft not in _INV:
        ns = nfft // 2 - 1
        nh = nfft // 2 + 1
        spec1 = _random_spectra(nfft + 3, 3, nfft)
        ones = np.ones((1, nh, nfft), dtype=np.complex128)
        base = [(0, 0), (1, 0), (2, 0)]
        f64, ext = fr.tables(spec1, ones, base, ns, nfft), fr.tables(spec1, ones, base, ns, nfft, extended=True)
        _INV[nfft] = (spec1, ext, [fr.yardstick(f64[p], ext[p]) for p in range(3)], [fr.norm2(spec1[p]) / nfft for p in range(3)])
    return _INV[nfft]


@pytest.mark.parametrize("count", ["1", "7", "8", "9", "rows", "generic9"])
@pytest.mark.parametrize("nfft", STATIC)
def test_inverse_pair_counts_over_the_xcd_partition(nfft, count, monkeypatch):
    """XCD x of the inverse column kernel takes the pairs [npairs x / 8, npairs (x + 1) / 8): with 1 and 7 pairs some ranges are empty, with
    8 every one holds one pair, with 9 one holds two; `rows` is one more pair than cu x 12 row lines hold, so that the row loop takes a
    second trip.  Pair t is (t % 3, (t // 3) % 4) over three random spectra and the four constant spectra 1, 2, 4, 8: its table is 2^q
    times the table of spectrum p, exactly, so every table has its own expected value from three extended-precision inverses.
    generic9: nine pairs through the general kernels."""
    generic = count.startswith("generic")
    if generic:
        monkeypatch.setenv("IMCOM_FFT_GENERIC", "1")
    else:
        monkeypatch.delenv("IMCOM_FFT_GENERIC", raising=False)
    ns, nh = nfft // 2 - 1, nfft // 2 + 1
    npairs = 9 if generic else (_cu() * 12 // ((ns + 1) // 2) + 1 if count == "rows" else int(count))
    spec1, ext, yards, n2 = _inverse_case(nfft)
    spec2 = np.ones((4, nh, nfft), dtype=np.complex128) * np.array([1.0, 2.0, 4.0, 8.0])[:, None, None]
    pairs = [(t % 3, (t // 3) % 4) for t in range(npairs)]
    got = _inverse(spec1, spec2, pairs, ns, nfft)
    worst = max(_ratio(got[t] / 2.0**q, ext[p], yards[p], n2[p]) for t, (p, q) in enumerate(pairs))
    _report(f"e inverse nfft={nfft} npairs={npairs} {'generic' if generic else 'static'}", worst)


# ---- f. odd sides and the dense neighbours, through the tophat filter -----------------------------------------------------------------
def _tophat_case(label, N, route_name):
    from pyimcom_amd import splitpsf as sp
    from pyimcom_amd._lib import MEM_HOST, check, default_context, lib, ptr

    n, width = N - 8, 1.0
    sz = sp._sizes(n, 3, width)
    assert (int(sz[0]), int(sz[1]), int(sz[2])) == (4, N, getattr(sp, route_name))
    cube = np.random.default_rng(N).standard_normal((3, n, n))
    cube[:, -1, -1] += 1.0
    out = np.full_like(cube, NAN)
    check(lib.imcom_splitpsf_tophat(default_context().handle, ptr(cube), 3, n, width, ptr(out), MEM_HOST))
    assert np.isfinite(out).all()
    want, ext = spref.tophatfilter(cube, width), spref.tophatfilter(cube, width, extended=True)
    ref_err = float(np.abs(want - ext).max())
    d, b = float(np.abs(out - want).max()), spref.bound(ref_err, want)
    print(f"fft-edges {label} N={N}: |device - reference| {d:.3e}  bound {b:.3e}  (ref_err {ref_err:.3e}, max |reference| {np.abs(want).max():.3e}), "
          f"|device - extended| / (bound / 10) = {10.0 * float(np.abs(out - ext).max()) / b:.3f}")
    assert out.shape == want.shape and out.dtype == np.float64
    assert d <= b


@pytest.mark.parametrize("N", ODD)
def test_odd_sides_through_the_tophat(N):
    """Forward and inverse complex line transforms at side N = n + 8 (width 1: a padding of 4), three planes riding as two complex ones
    (2 N lines: a ragged last workgroup); sinc(u) sinc(v) >= 0.4 over the whole band, so no bin is filtered away."""
    _tophat_case("f tophat lines", N, "ROUTE_LINES")


@pytest.mark.parametrize("N", [11, 14, 447, 448, 449])
def test_dense_fallback_at_its_padding_edges(N):
    """The dense-DFT engine of fft.hip at the smallest sides no plan takes (11, 14) and around 448 = 64 x 7: 2 N = 896 is a multiple of the
    GEMM tile (128) there, the padded matrix has no zero margin, and the sides one below and one above have the widest and the
    narrowest one."""
    assert N not in fr.plan_sides() and (N != 448 or (2 * N) % 128 == 0)
    _tophat_case("f tophat dense", N, "ROUTE_DENSE")


# ---- g. refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft,ns", [(14, 5), (1026, 5), (15, 5), (60, 31), (512, 257)])
def test_sides_without_a_plan_are_refused(nfft, ns):
    from pyimcom_amd._lib import lib

    torch, ctx = _dev()
    assert int(lib.imcom_psf_spectra_size(ns, nfft)) == 0
    t = torch.as_tensor(_psfs(1, 2, ns), device="cuda:0")
    spec = torch.full((2, 2 * (nfft // 2 + 1) * nfft), -7.0, dtype=torch.float64, device="cuda:0")
    status = lib.imcom_psf_spectra(ctx.handle, _dp(t), 2, ns, nfft, _dp(spec))
    assert status < 0 and len(lib.imcom_last_error()) > 0
    torch.cuda.synchronize()
    assert bool((spec == -7.0).all())
