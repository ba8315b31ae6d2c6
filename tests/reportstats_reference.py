"""Numpy restatement of the validation report's statistics (reference src/pyimcom/diagnostics/layer_diagnostics.py:24-64, 105-142;
src/pyimcom/diagnostics/dynrange.py:68-79, 140-163, 211-239) and the inputs of their golden vectors.  tests/golden/make_golden_reportstats.py
runs the reference's own statements on these inputs; tests/test_reportstats_host.py holds this restatement against what they gave."""

import numpy as np

PCTILES = [0, 0.01, 0.1, 1, 5, 25, 50, 75, 95, 99, 99.9, 99.99, 100]
RING_Q = [1, 5, 25, 50, 75, 95, 99]
NS, D, NBLOCK, NLAYERS, MISSING = 32, 4, 3, 3, (1, 2)  # a mosaic of 3 x 3 blocks of 40^2 frames; block (ibx, iby) = (1, 2) has no file
N_STAR_FRAME, RPIX, BD = 96, 9, 10
SIGMA_UNIT, NEFF_UNIT = ("-0.1mB", "-10000*log10(Sigma)"), ("0.02mB", "50000*log10(Neff)")  # UNIT and its comment (coadd.py:2249-2303)


def mosaic():
    """{(ibx, iby): float32 [NLAYERS, 40, 40]} without the missing block.  Layer 0 is noise, layer 1 a few levels (long ties, both signs of
    zero), layer 2 mostly zero with a heavy tail and values from 1e-30 to 1e30 (many first digits)."""
    rng = np.random.default_rng(20240612)
    n = NS + 2 * D
    out = {}
    for iby in range(NBLOCK):
        for ibx in range(NBLOCK):
            if (ibx, iby) == MISSING:
                continue
            f = np.zeros((NLAYERS, n, n), dtype=np.float32)
            f[0] = rng.standard_normal((n, n)).astype(np.float32)
            f[1] = (np.round(rng.standard_normal((n, n)) * 2) / 4).astype(np.float32)
            f[1][::5, ::3] = -0.0
            tail = rng.uniform(size=(n, n)) < 0.4
            f[2][tail] = (rng.choice([-1.0, 1.0], size=int(tail.sum())) * 10.0 ** rng.uniform(-30, 30, size=int(tail.sum()))).astype(np.float32)
            out[(ibx, iby)] = f
    return out


def layer_array(frames, ilayer):
    """layer_diagnostics.py:114, 124-142: the flat array of one layer; a missing block leaves its zeros."""
    data = np.zeros(((NS * NBLOCK) ** 2,), dtype=np.float32)
    for iby in range(NBLOCK):
        for ibx in range(NBLOCK):
            if (ibx, iby) not in frames:
                continue
            chunk = iby * NBLOCK + ibx
            x_ = frames[(ibx, iby)][ilayer]
            if D > 0:
                x_ = x_[D:-D, D:-D]
            data[chunk * NS * NS:(chunk + 1) * NS * NS] = x_.ravel()
    return data


def percentiles_of_sorted(arr, pctiles):
    """layer_diagnostics.py:49-57 on an array that is sorted already."""
    target = np.zeros(len(pctiles), dtype=np.float32)
    nsize = arr.size
    for k in range(len(pctiles)):
        pos = (nsize - 1) * pctiles[k] / 100.0
        p1 = max(int(np.floor(pos)), 0)
        if p1 >= nsize - 1:
            p1 = nsize - 2
        frac = np.clip(pos - p1, 0.0, 1.0)
        target[k] = (1 - frac) * arr[p1] + frac * arr[p1 + 1]
    return target


def layer_percentiles(frames):
    return np.stack([percentiles_of_sorted(np.sort(layer_array(frames, i), kind="mergesort"), PCTILES) for i in range(NLAYERS)])


def star_frame():
    """(starmap float32 [96, 96], x, y float64 [12], sigma codes int16, neff codes uint16).  Stars: integer and half-integer positions (the
    squared radius is an exact square at many pixels: 3-4-5, 6-8-10), boxes clipped at each of the four edges, one wholly off the frame,
    two whose boxes overlap, and plain ones."""
    rng = np.random.default_rng(777)
    n = N_STAR_FRAME
    x = np.array([30.0, 60.5, 2.3, 94.2, 50.7, 48.125, -30.5, 40.25, 45.0, 20.9, 75.0, 70.5])
    y = np.array([30.0, 20.5, 50.1, 47.6, 1.5, 95.0, 40.0, 40.5, 43.0, 70.3, 75.5, 80.0])
    yy, xx = np.mgrid[0:n, 0:n]
    starmap = rng.standard_normal((n, n)) * 0.5
    for xs, ys in zip(x, y):
        starmap += 3000.0 * np.exp(-((xx - xs) ** 2 + (yy - ys) ** 2) / (2 * 1.2 ** 2))
    starmap = starmap.astype(np.float32)
    sigma = np.round(-10000 * np.log10(rng.uniform(0.3, 2.5, size=(n, n)))).astype(np.int16)
    sigma[BD, BD], sigma[BD, BD + 1], sigma[n - BD - 1, n - BD - 1], sigma[0, 0] = -32768, 32767, 0, -32768  # (the last one outside the crop)
    neff = np.round(50000 * np.log10(rng.uniform(1.0, 14.0, size=(n, n)))).astype(np.uint16)
    neff[BD, BD], neff[BD + 1, BD], neff[n - BD - 1, BD] = 0, 65535, 50000
    return starmap, x, y, sigma, neff


def unit_to_bels(unit, comment):
    """outimage_utils/helper.py:36-48, 74-78 for the units this project writes ("<number>mB")."""
    assert unit.endswith("mB")
    val = float(unit[:-2]) * 1e-3
    if val > 0 and comment[0] == "-":
        val = -val
    return val


def ring_values(starmap, x, y, rpix):
    """dynrange.py:212-228 as a direct loop over stars and pixels: the values of ring j in the reference's order."""
    n = starmap.shape[-1]
    vals = [[] for _ in range(rpix)]
    for xs, ys in zip(x, y):
        xmin = int(np.clip(np.floor(xs).astype(np.int16) - rpix - 1, 0, n))
        xmax = int(np.clip(np.ceil(xs).astype(np.int16) + rpix + 1, 0, n))
        ymin = int(np.clip(np.floor(ys).astype(np.int16) - rpix - 1, 0, n))
        ymax = int(np.clip(np.ceil(ys).astype(np.int16) + rpix + 1, 0, n))
        per = [[] for _ in range(rpix)]
        for row in range(ymin, ymax):
            for col in range(xmin, xmax):
                r = int(np.floor(np.sqrt((col - xs) ** 2 + (row - ys) ** 2)))
                if r < rpix:
                    per[r].append(starmap[row, col])
        for j in range(rpix):
            vals[j] += per[j]
    return [np.asarray(v, dtype=np.float32) for v in vals]


def histogram(codes, bels, half, width, nbins, bd, nscale=1):
    """dynrange.py:142-150 (half) / 155-163: (counts [nbins], size, off scale high) of one coded map."""
    n = codes.shape[-1]
    c = codes[bd:n - bd, bd:n - bd]
    v = 10 ** (0.5 * bels * c) if half else 10 ** (bels * c * nscale)
    counts = np.array([np.count_nonzero(np.logical_and(v / width >= j, v / width < j + 1)) for j in range(nbins)], dtype=np.float64)
    return counts, float(np.size(v)), float(np.count_nonzero(v >= width * nbins))
