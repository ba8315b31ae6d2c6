"""Reference helpers of the dense-LA edge tests (tests/test_gpu_la_edges.py): symmetric matrices whose spectra are
known exactly or to far more than float64 accuracy, and a linear solve refined with residuals in extended precision.
Plain numpy / scipy / mpmath; the CPU suite checks the helpers themselves (tests/test_la_reference.py)."""

import numpy as np
from scipy.linalg import cho_factor, cho_solve

EPS = 2.220446049250313e-16
LD = np.longdouble


# ------------------------------------------------------------------------------------------------ known spectra
def toeplitz_2_1(n):
    """tridiag(-1, 2, -1): lambda_k = 2 - 2 cos(k pi / (n + 1)), k = 1..n (ascending); exact integer entries."""
    A = 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    k = np.arange(1, n + 1, dtype=LD)
    lam = 2 - 2 * np.cos(k * LD(np.pi) / (n + 1))
    return A, np.sort(lam.astype(np.float64))


def clement(n):
    """Clement / Kac matrix (symmetric form): zero diagonal, off-diagonal sqrt(k (n - k)); eigenvalues -(n-1), -(n-3), ..., n-1.
    The off-diagonal entries are rounded once (relative 1.1e-16): the spectrum moves by at most eps * max|lambda|."""
    k = np.arange(1, n, dtype=np.float64)
    b = np.sqrt(k * (n - k))
    A = np.diag(b, 1) + np.diag(b, -1)
    return A, np.arange(-(n - 1), n, 2, dtype=np.float64)


def reflectors(n, count, rng):
    """`count` Householder reflectors H = I - 2 v v^T / v^T v of small-integer vectors v (as the list of v)."""
    out = []
    for _ in range(count):
        v = rng.integers(-3, 4, n).astype(np.float64)
        if not v.any():
            v[rng.integers(n)] = 1.0
        out.append(v)
    return out


def with_spectrum(w, rng, count=6, blocks=None):
    """Dense symmetric V diag(w) V^T with V = H_k ... H_1, formed in long double and rounded once: its eigenvalues are w to within
    n eps max|w| / 2 (the rounding) and its tridiagonal form is full.  blocks = [(lo, hi), ...]: separate reflectors act on rows
    lo..hi-1 of each block only, so the matrix is block-diagonal.  Returns (A, V) with V rounded to float64."""
    w = np.asarray(w, dtype=np.float64)
    n = w.size
    M = np.diag(w.astype(LD))
    V = np.eye(n, dtype=LD)
    for lo, hi in blocks or [(0, n)]:
        for v in reflectors(hi - lo, count, rng):
            u = np.zeros(n, dtype=LD)
            u[lo:hi] = v
            c = LD(2) / (u @ u)
            M = M - np.outer(u, c * (u @ M))  # H M
            M = M - np.outer(M @ u, c * u)  # (H M) H
            V = V - np.outer(u, c * (u @ V))  # H V
    M = 0.5 * (M + M.T)
    return M.astype(np.float64), V.astype(np.float64)


def wilkinson_plus(n):
    """Wilkinson W_n^+ (n odd): diag |(n-1)/2 - i|, off-diagonal 1 -- eigenvalues in pairs agreeing to ~1e-14 at the top."""
    h = (n - 1) // 2
    return np.diag(np.abs(h - np.arange(n)).astype(np.float64)) + np.eye(n, k=1) + np.eye(n, k=-1)


def glued_wilkinson(sizes, delta):
    """W_k^+ for k in `sizes` on the diagonal, glued by off-diagonal entries `delta`: clusters of near-degenerate eigenvalues."""
    n = sum(sizes)
    A = np.zeros((n, n))
    o = 0
    for k in sizes:
        A[o:o + k, o:o + k] = wilkinson_plus(k)
        if o:
            A[o - 1, o] = A[o, o - 1] = delta
        o += k
    return A


def mp_eigvalsh(A, dps=30):
    """Eigenvalues (ascending) of a small symmetric float64 matrix by mpmath at `dps` digits, rounded to float64."""
    import mpmath

    n = A.shape[0]
    with mpmath.workdps(dps):
        M = mpmath.matrix(n, n)
        for i in range(n):
            for j in range(n):
                M[i, j] = mpmath.mpf(float(A[i, j]))
        E = mpmath.eigsy(M, eigvals_only=True)
        return np.sort(np.array([float(E[i]) for i in range(n)]))


# ------------------------------------------------------------------------------------------------ refined solve
def gaussian_overlap(n, rng, width=12.0, r2scale=3.0, scale=1.0):
    """exp(-|r_i - r_j|^2 / r2scale) on n uniform points of a width x width square (the PSF-overlap form of the LA tests); with
    a cross-correlation factory for m output points."""
    pts = rng.uniform(0, width, (n, 2))
    A = scale * np.exp(-((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1) / r2scale)

    def mbhalf(m):
        outp = rng.uniform(0.15 * width, 0.85 * width, (m, 2))
        return scale * np.exp(-((outp[:, None, :] - pts[None, :, :]) ** 2).sum(-1) / (r2scale + 0.5))

    return A, mbhalf


def solve_refined(A, kappa, B, steps=2):
    """X = (A + kappa I)^-1 B: float64 Cholesky (scipy cho_solve) and `steps` steps of iterative refinement whose residuals
    B - (A + kappa I) X are formed in long double.  Forward error ~ eps + cond eps_longdouble (1e-8 at cond 1e11; cond eps < 1),
not cond eps as the plain solve."""
    n = A.shape[0]
    AA = A + kappa * np.eye(n)
    F = cho_factor(AA, lower=True, check_finite=False)
    X = cho_solve(F, B, check_finite=False)
    AL = A.astype(LD)
    AL[np.diag_indices(n)] += LD(kappa)
    BL = B.astype(LD)
    XL = X.astype(LD)
    for _ in range(steps):
        R = BL - AL @ XL
        XL = XL + cho_solve(F, R.astype(np.float64), check_finite=False).astype(LD)
    return XL


def solve_refined_lu(A, kappa, B, steps=2):
    """solve_refined for A + kappa I that is indefinite but well conditioned: LU with partial pivoting (scipy lu_factor) in
    place of the Cholesky factorisation, the same long-double residuals."""
    from scipy.linalg import lu_factor, lu_solve

    n = A.shape[0]
    F = lu_factor(A + kappa * np.eye(n), check_finite=False)
    AL = A.astype(LD)
    AL[np.diag_indices(n)] += LD(kappa)
    BL = B.astype(LD)
    XL = lu_solve(F, B, check_finite=False).astype(LD)
    for _ in range(steps):
        R = BL - AL @ XL
        XL = XL + lu_solve(F, R.astype(np.float64), check_finite=False).astype(LD)
    return XL


def chol_maps_refined(A, mBhalf, C, kappaC):
    """lakernel.CholKernel._call_single_kappa (one kappa node) from the refined solve: T [m][n] (long double), UC, Sigma, and the
    scale (kappa N + |D|) / C of the two terms whose difference UC is."""
    kap = kappaC * C
    T = solve_refined(A, kap, mBhalf.T).T
    D = np.einsum("ai,ai->a", mBhalf.astype(LD), T)
    N = np.einsum("ai,ai->a", T, T)
    UC = 1 - (kap * N + D) / C
    return T, UC.astype(np.float64), N.astype(np.float64), ((kap * N + np.abs(D)) / C).astype(np.float64)


def cond_spd(A, kappa):
    """2-norm condition number of A + kappa I from numpy's eigenvalues (A symmetric, A + kappa I positive definite)."""
    w = np.linalg.eigvalsh(A)
    return (w[-1] + kappa) / (w[0] + kappa)
