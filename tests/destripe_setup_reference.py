"""Reference for the destripe set-up made from WCSs (seam 21), independent of pyimcom_amd: ``Sca_img``'s effective gain (reference
src/pyimcom/imdestripe.py:281-297 with ``get_coordinates(pad=2.0)``, 451-474) restated (1) in float64 numpy over tests/wcs_reference.py's
``np_pix2world`` -- pinned with ``==`` to the reference's own statements run over the same chain (tests/golden/destripe_setup.npz, written
by tests/golden/make_golden_destripe_setup.py) -- and (2) in 40-digit arithmetic over ``mp_pix2world``, and the rule of ``get_neighbors``
(1225-1228).

The quirk both keep (292-293): the reference stacks its four derivative images, transposes the whole stack -- which also swaps the two
pixel axes -- and reshapes it to one 2 x 2 matrix a pixel, so the determinants come back transposed against ``dec``:
``g_eff[i, j] = 1 / (|det at pixel (row j, column i)| cos(dec at pixel (row i, column j)))``."""

import numpy as np

from tests import wcs_reference as R


def frame_axis(nside):
    """The pixel coordinates of get_coordinates(pad=2.0) on either axis: -1, 0, .., nside."""
    return np.arange(nside + 2, dtype=np.float64) - 1.0


def np_frame(desc, tab, nside):
    """(ra, dec) [nside + 2, nside + 2] in degrees, axes (y, x)."""
    ax = frame_axis(nside)
    x, y = np.meshgrid(ax, ax, indexing="xy")
    ra, dec = R.np_pix2world(desc, tab, x.ravel(), y.ravel(), 0)
    return ra.reshape(nside + 2, nside + 2), dec.reshape(nside + 2, nside + 2)


def np_effective_gain(desc, tab, nside, dtype=np.float64):
    """The gain [nside, nside] in float64, cast to ``dtype`` at the end (the reference assigns it into an array of use_output_float)."""
    ra, dec = np_frame(desc, tab, nside)
    d_dx = lambda f: (f[1:-1, 2:] - f[1:-1, :-2]) / 2  # noqa: E731
    d_dy = lambda f: (f[2:, 1:-1] - f[:-2, 1:-1]) / 2  # noqa: E731
    jac = np.empty((nside, nside, 2, 2))
    jac[..., 0, 0], jac[..., 0, 1], jac[..., 1, 0], jac[..., 1, 1] = d_dx(ra), d_dy(ra), d_dx(dec), d_dy(dec)
    det = np.linalg.det(jac)  # [row, column]; the reference's det_mat is its transpose
    g = 1 / (np.abs(det.T) * np.cos(np.deg2rad(dec[1:-1, 1:-1])))
    return g.astype(dtype)


def mp_effective_gain(P, tab, nside):
    """The same statements in 40 digits from the header values, rounded once to float64."""
    mp = R._mp()
    ax = frame_axis(nside)
    W = nside + 2
    ra = [[None] * W for _ in range(W)]
    dec = [[None] * W for _ in range(W)]
    for j in range(W):
        for i in range(W):
            ra[j][i], dec[j][i] = R.mp_pix2world(P, tab, ax[i], ax[j], 0)
    det = [[None] * nside for _ in range(nside)]
    for r in range(nside):
        for c in range(nside):
            rx, ry = (ra[r + 1][c + 2] - ra[r + 1][c]) / 2, (ra[r + 2][c + 1] - ra[r][c + 1]) / 2
            dx, dy = (dec[r + 1][c + 2] - dec[r + 1][c]) / 2, (dec[r + 2][c + 1] - dec[r][c + 1]) / 2
            det[r][c] = rx * dy - ry * dx
    out = np.zeros((nside, nside))
    for i in range(nside):
        for j in range(nside):
            out[i, j] = float(1 / (abs(det[j][i]) * mp.cos(dec[i + 1][j + 1] * mp.pi / 180)))
    return out


def neighbors_of(ov_mat, overlap_thresh):
    """get_neighbors' rule (1225-1228) on an overlap matrix."""
    n = len(ov_mat)
    return {k: [j for j in range(n) if ov_mat[k, j] >= overlap_thresh and j != k] for k in range(n)}
