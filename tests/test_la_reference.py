"""The reference helpers of tests/test_gpu_la_edges.py checked on their own (CPU only): the known spectra are what numpy and
mpmath find, and the refined solve is accurate to a few eps where a plain float64 solve is not."""

import numpy as np

from tests import la_reference as ref


def test_known_spectra():
    rng = np.random.default_rng(1)
    for n in (1, 2, 7, 40):
        for A, w in (ref.toeplitz_2_1(n), ref.clement(n)):
            assert np.array_equal(A, A.T)
            assert np.abs(np.linalg.eigvalsh(A) - w).max() <= 10 * n * ref.EPS * np.abs(w).max()
    w = np.concatenate([np.ones(5), np.linspace(-2.0, 3.0, 30)])
    A, V = ref.with_spectrum(w, rng)
    assert np.array_equal(A, A.T) and np.abs(np.tril(A, -2)).min() >= 0 and np.count_nonzero(np.tril(A, -2)) > 300  # dense
    assert np.abs(np.linalg.eigvalsh(A) - np.sort(w)).max() <= 10 * w.size * ref.EPS * 3.0
    assert np.abs(V.T @ V - np.eye(w.size)).max() <= 4 * ref.EPS and np.abs(A @ V - V * w).max() <= 10 * w.size * ref.EPS * 3.0
    A, _ = ref.with_spectrum(np.arange(10.0), rng, blocks=[(0, 4), (4, 10)])
    assert not A[:4, 4:].any() and np.abs(np.linalg.eigvalsh(A) - np.arange(10.0)).max() <= 1e-13


def test_wilkinson_spectra_vs_mpmath():
    W = ref.wilkinson_plus(21)
    w = ref.mp_eigvalsh(W)
    assert abs(w[-1] - 10.7461941829033) < 1e-12  # W21+'s largest eigenvalue (Wilkinson, The Algebraic Eigenvalue Problem)
    assert 0 < w[-1] - w[-2] < 1e-13  # the top pair is near-degenerate
    G = ref.glued_wilkinson([13, 13, 13], 1e-12)
    assert G.shape == (39, 39) and G[12, 13] == 1e-12 and G[13, 12] == 1e-12
    g = ref.mp_eigvalsh(G)
    assert np.abs(np.linalg.eigvalsh(G) - g).max() <= 40 * 39 * ref.EPS * np.abs(g).max()


def test_refined_solve_vs_mpmath():
    """At cond(A + kappa I) ~ 1e11 the refined solution agrees with a 40-digit solve to eps + cond eps_longdouble (1e-8 at most,
    against the c cond eps ~ 1e-3 the GPU tests allow the kernel); a plain float64 Cholesky solve is off by about cond eps."""
    import mpmath
    from scipy.linalg import cho_factor, cho_solve

    rng = np.random.default_rng(30)
    A, mb = ref.gaussian_overlap(30, rng, width=2.5)
    B = mb(3).T.copy()
    kap = np.linalg.eigvalsh(A)[-1] / 1e11
    cond = ref.cond_spd(A, kap)
    assert 1e10 < cond < 1e12
    X = ref.solve_refined(A, kap, B).astype(np.float64)
    with mpmath.workdps(40):
        M = mpmath.matrix(A.tolist())
        for i in range(30):
            M[i, i] += mpmath.mpf(float(kap))
        Xm = np.array([[float(v) for v in mpmath.lu_solve(M, mpmath.matrix(B[:, j].tolist()))] for j in range(B.shape[1])]).T
    scale = np.abs(Xm).max()
    eps_ld = float(np.finfo(ref.LD).eps)
    assert eps_ld < 1e-18  # (x86 80-bit long double: the residuals carry 11 more bits than float64)
    err = np.abs(X - Xm).max()
    assert err <= (8 * ref.EPS + 2 * cond * eps_ld) * scale
    X0 = cho_solve(cho_factor(A + kap * np.eye(30), lower=True), B)
    assert np.abs(X0 - Xm).max() > 100 * err  # (the refinement is needed: the plain solve is far off)
    # the maps from the refined T
    T, UC, N, sc = ref.chol_maps_refined(A, B.T.copy(), 1.0, kap)
    assert np.allclose(T.astype(np.float64), Xm.T, rtol=0, atol=(8 * ref.EPS + 2 * cond * eps_ld) * scale)
    assert np.allclose(N, (Xm**2).sum(0), rtol=4 * (8 * ref.EPS + 2 * cond * eps_ld)) and np.all(sc > 0)
