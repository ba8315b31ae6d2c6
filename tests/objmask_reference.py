"""The bright-object mask of the destripe set-up restated with numpy alone (no scipy): what ``apply_object_mask`` of the reference
(src/pyimcom/imdestripe.py:781-872) computes, with a sort for the median, shift-and-or for the dilations and a frontier sweep for the
propagation.  tests/test_objmask_host.py pins it to the reference's own outputs (tests/golden/objmask.npz) bit for bit; the device tests
use it for shapes beyond the fixture.  Also the synthetic images both the generator and the tests are made of."""

import numpy as np


def median(a):
    """``np.median`` of all elements by a full sort: NaN if any element is NaN or there is none; the mean of the two middle elements, formed
    in the array's type, for an even count."""
    a = np.asarray(a).ravel()
    if a.size == 0 or np.isnan(a).any():
        return a.dtype.type(np.nan)
    s = np.sort(a)
    mid = s[(a.size - 1) // 2: a.size // 2 + 1]
    with np.errstate(over="ignore"):
        return np.mean(mid)


def dilate(mask, r):
    """Box dilation: a pixel is set when any pixel within ``r`` rows and ``r`` columns is; nothing is set outside the image."""
    mask = np.asarray(mask, dtype=bool)
    H, W = mask.shape
    pad = np.zeros((H + 2 * r, W + 2 * r), dtype=bool)
    pad[r:r + H, r:r + W] = mask
    rows = np.zeros_like(pad)
    for d in range(-r, r + 1):
        rows |= np.roll(pad, d, axis=1)  # (the pad is r wide: nothing wraps into the image)
    out = np.zeros_like(pad)
    for d in range(-r, r + 1):
        out |= np.roll(rows, d, axis=0)
    return out[r:r + H, r:r + W]


def propagate(seed, grow):
    """The seed plus every grow pixel that a 4-connected path of grow pixels joins to a seed pixel or to a 4-neighbour of one."""
    state = np.array(seed, dtype=bool)
    grow = np.asarray(grow, dtype=bool)
    H, W = state.shape
    fy, fx = np.nonzero(state)
    while fy.size:
        ny = np.concatenate([fy - 1, fy + 1, fy, fy])
        nx = np.concatenate([fx, fx, fx - 1, fx + 1])
        ok = (ny >= 0) & (ny < H) & (nx >= 0) & (nx < W)
        ny, nx = ny[ok], nx[ok]
        new = grow[ny, nx] & ~state[ny, nx]
        ny, nx = ny[new], nx[new]
        state[ny, nx] = True
        lin = np.unique(ny * W + nx)
        fy, fx = lin // W, lin % W
    return state


def apply_object_mask(image, mask=None, threshold_m=0, threshold_c=0.3, inplace=False, type="fits", details=None):
    """(image_out, neighbor_mask) as the reference returns them; ``details`` (a dict) receives the intermediates under the reference's
    names."""
    d = details if details is not None else {}
    if isinstance(mask, np.ndarray):
        neighbor = mask
    else:
        if type == "jwst":
            valid = np.isfinite(image)
            if not valid.any():
                high = np.zeros(image.shape, dtype=bool)
                d["seed_threshold"] = d["grow_threshold"] = 0.0
            else:
                kept = image[valid]
                for _ in range(3):
                    bkg = median(kept)
                    sigma = 1.4826 * median(np.abs(kept - bkg))
                    if sigma <= 0:
                        break
                    inside = np.abs(kept - bkg) < 3.0 * sigma
                    if np.count_nonzero(inside) < 100:
                        break
                    kept = kept[inside]
                bkg = median(kept)
                mad = median(np.abs(kept - bkg))
                sigma = 1.4826 * mad
                if not np.isfinite(sigma) or sigma <= 0:
                    sigma = np.std(kept) if kept.size > 1 else 0.0
                seed_threshold = max(threshold_c, 6.0 * sigma)
                grow_threshold = max(0.5 * threshold_c, 2.5 * sigma)
                with np.errstate(invalid="ignore", over="ignore"):
                    resid = np.where(valid, image - bkg, np.zeros((), dtype=image.dtype))
                seed = valid & (resid >= seed_threshold)
                cand = valid & (resid >= grow_threshold)
                grown = propagate(seed, cand)
                high = dilate(grown, 2)  # a 3 x 3 box, twice
                d.update(bkg=bkg, mad=mad, sigma=sigma, seed_threshold=seed_threshold, grow_threshold=grow_threshold, seed_mask=seed, grow_candidates=cand,
                         grown_mask=grown, n_clip=kept.size)
        else:
            median_val = median(image)
            with np.errstate(invalid="ignore"):
                high = image >= threshold_m * median_val + threshold_c
            d["median_val"] = median_val
        d["high_value_mask"] = high
        neighbor = dilate(high, 2)  # a 5 x 5 box
    if inplace:
        image[neighbor] = 0
        return image, neighbor
    return np.where(neighbor, 0, image), neighbor


# ---- synthetic scenes ----
def scene(shape, dtype, seed, nsrc=6, nonfinite=0, step=1.0 / 64):
    """Sky noise quantised to ``step`` (ties in every order statistic), Gaussian sources of several brightnesses, two of them on the
    borders, and ``nonfinite`` pixels of +inf, -inf and NaN in turn."""
    rng = np.random.default_rng(seed)
    H, W = shape
    img = 0.05 + 0.04 * rng.standard_normal(shape)
    yy, xx = np.mgrid[:H, :W]
    cy = np.concatenate([[0, H - 1], rng.integers(5, H - 5, size=nsrc)])
    cx = np.concatenate([[W // 3, W - 1], rng.integers(5, W - 5, size=nsrc)])
    for k, (y, x) in enumerate(zip(cy, cx)):
        img += (0.6 + 1.7 * k) * np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2.0 * (1.0 + 0.4 * k) ** 2))
    img = (np.round(img / step) * step).astype(dtype)
    for k in range(nonfinite):
        img[rng.integers(0, H), rng.integers(0, W)] = (np.inf, -np.inf, np.nan)[k % 3]
    return img


def fits_threshold(image, threshold_m, threshold_c):
    """The threshold of the plain route as numpy forms it (a scalar of numpy's choice of type)."""
    return threshold_m * np.median(image) + threshold_c


def fits_scene(shape=(150, 203), seed=3, threshold_m=0, threshold_c=0.3):
    """A float32 scene with one pixel exactly on the threshold (``>=`` includes it) and its neighbour one ulp below."""
    img = scene(shape, np.float32, seed)
    thr = np.float32(fits_threshold(img, threshold_m, threshold_c))
    y, x = shape[0] // 2, 20
    assert img[y - 6:y + 7, x - 6:x + 7].max() < thr  # quiet sky around: the two pixels decide their neighbourhood alone
    img[y, x] = thr
    img[y + 40, x] = np.nextafter(thr, np.float32(-np.inf))
    assert np.float32(fits_threshold(img, threshold_m, threshold_c)) == thr
    return img


def golden_cases():
    """name -> (image, threshold_m, threshold_c, type): the cases of tests/golden/objmask.npz."""
    const = np.full((20, 23), 1.25, dtype=np.float64)
    bad = np.full((10, 12), np.nan, dtype=np.float32)
    bad[::3, ::2] = np.inf
    bad[1::3, 1::2] = -np.inf
    return {
        "fits_m0": (fits_scene(), 0, 0.3, "fits"),
        "fits_m15": (fits_scene(threshold_m=15), 15, 0.3, "fits"),
        "asdf_f64": (scene((64, 70), np.float64, 5), 2.0, 0.1, "asdf"),
        "jwst_f64": (scene((96, 120), np.float64, 7, nonfinite=9), 0, 0.3, "jwst"),
        "jwst_f32": (scene((96, 120), np.float32, 8, nonfinite=6), 0, 0.05, "jwst"),
        "jwst_const": (const, 0, 0.3, "jwst"),
        "jwst_small": (scene((8, 8), np.float64, 9, nsrc=0), 0, 0.3, "jwst"),
        "jwst_nonfinite": (bad, 0, 0.3, "jwst"),
    }
