"""The hand-written dense LA at its edges: imcom_eigh (csrc/tridiag.hip) against exact or high-precision spectra, and
imcom_solve_chol (blocked Cholesky) against a refined solve, at the sizes where their paths switch -- 128-row panels and
tiles, the 96-row limit of the one-after-the-other QR sweeps, ragged batches with padded rows, 1..8 kappa nodes -- and the
Cholesky repair with stamps on both sides of the 1024-row switch between the eigensolver and the subspace iteration.  Direct
C-ABI calls, so that ragged n and ldn are the test's; the padding of every input is NaN and must not reach an output."""

import ctypes as C

import numpy as np
import pytest

from tests import la_reference as ref

pytestmark = pytest.mark.gpu

EPS = ref.EPS
RTOL_MAP, ATOL_MAP = 1e-5, 1e-9  # UC, Sigma (tests/test_gpu_routines.py)
SENT = 7.0  # outputs are pre-filled with this: what the library must overwrite (or zero) is seen to be written


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _lib():
    from pyimcom_amd._lib import MEM_HOST, default_context, lib

    return lib, default_context().handle, MEM_HOST


def _check(status):
    from pyimcom_amd._lib import check

    check(status)


# ------------------------------------------------------------------------------------------------ imcom_eigh
C_EIG = 30  # every eigh bound below: c n eps (||A|| = max |lambda|)


def _eigh(mats, ldn):
    """imcom_eigh on a ragged batch: mats[s] is n_s x n_s (n_s may be 0), A padded with NaN to ldn."""
    lib, ctx, host = _lib()
    batch = len(mats)
    ns = np.array([m.shape[0] for m in mats], np.int32)
    A = np.full((batch, ldn, ldn), np.nan)
    for s, M in enumerate(mats):
        A[s, : M.shape[0], : M.shape[0]] = M
    A0 = A.copy()
    lam = np.full((batch, ldn), SENT)
    Q = np.full((batch, ldn, ldn), SENT)
    _check(lib.imcom_eigh(ctx, batch, _p(ns), ldn, _p(A), _p(lam), _p(Q), host))
    assert np.array_equal(A, A0, equal_nan=True)  # the input is not modified
    return lam, Q


def _check_eig(A, lam_true, lam, Q, tag, vectors=None):
    """lam [ldn], Q [ldn][ldn] of one stamp against the exact spectrum lam_true of its n x n matrix A.  vectors = (V, groups):
    V the exact eigenvectors (columns, in the order of lam_true's unsorted source), groups = lists of ascending indices of
    multiple / clustered eigenvalues and their gap to the rest: the computed span must be the exact one."""
    n = A.shape[0]
    assert np.isfinite(lam).all() and np.isfinite(Q).all(), tag
    assert np.all(lam[n:] == 0) and np.all(Q[n:, :] == 0) and np.all(Q[:, n:] == 0), tag  # nothing outside the leading block
    if n == 0:
        return
    w, V = lam[:n], Q[:n, :n]
    nrm = np.abs(lam_true).max()
    tol = C_EIG * n * EPS
    assert np.all(np.diff(w) >= 0), tag
    err = np.abs(w - lam_true).max()
    assert err <= tol * nrm, (tag, err / (n * EPS * max(nrm, 1e-300)))
    orth = np.abs(V.T @ V - np.eye(n)).max()
    assert orth <= tol, (tag, orth / (n * EPS))
    res = np.abs(A @ V - V * w).max()
    assert res <= tol * nrm, (tag, res / (n * EPS * max(nrm, 1e-300)))
    if vectors is not None:
        Vx, groups = vectors
        for idx, gap in groups:
            X = Vx[:, idx]  # exact basis of the eigenspace
            Y = V[:, idx]
            off = np.abs(Y - X @ (X.T @ Y)).max()  # component of the computed vectors outside it
            assert off <= tol * nrm / gap, (tag, off * gap / (n * EPS * nrm))


SIZES = (1, 2, 3, 95, 96, 97, 127, 128, 129, 255, 257)


def _spectrum_cases(n, rng):
    """(kind, A, exact ascending eigenvalues, vectors-or-None) for one size."""
    out = []
    A, w = ref.toeplitz_2_1(n)
    out.append(("toeplitz", A, w, None))
    A, w = ref.clement(n)
    out.append(("clement", A, w, None))
    out.append(("zero", np.zeros((n, n)), np.zeros(n), None))
    c = -2.5 if n % 2 else 1.0
    out.append(("cI", c * np.eye(n), np.full(n, c), None))
    w = np.linspace(-3.0, 5.0, n) if n > 1 else np.array([0.75])
    out.append(("diag_scrambled", np.diag(rng.permutation(w)), np.sort(w), None))
    eta = 4e-14  # weakly coupled equal diagonal: I + eta tridiag(1, 0, 1) -- eigenvalues 1 + 2 eta cos(k pi / (n + 1)), a few eps apart
    k = np.arange(1, n + 1, dtype=ref.LD)
    w = np.sort((1 + 2 * ref.LD(eta) * np.cos(k * ref.LD(np.pi) / (n + 1))).astype(np.float64))
    out.append(("weak_coupling", np.eye(n) + eta * (np.eye(n, k=1) + np.eye(n, k=-1)), w, None))
    g = 10.0 ** (-17.0 * np.linspace(0.0, 1.0, n))  # graded, semi-definite to 1e-17 of the largest (the PSF-overlap regime)
    A, _ = ref.with_spectrum(rng.permutation(g), rng)
    out.append(("graded", A, np.sort(g), None))
    v = np.linspace(0.1, 2.0, n // 2)
    w = np.concatenate([v, -v] + ([np.zeros(1)] if n % 2 else []))
    A, _ = ref.with_spectrum(w, rng)
    out.append(("pm_pairs", A, np.sort(w), None))
    if n >= 2:  # two blocks: the tridiagonal form splits in the middle -- an exact zero off-diagonal inside a chunk
        h = n // 2
        w = np.concatenate([np.linspace(0.5, 2.0, h), np.linspace(-1.0, 1.7, n - h) + 1e-3])
        A, _ = ref.with_spectrum(w, rng, blocks=[(0, h), (h, n)])
        out.append(("block_diag", A, np.sort(w), None))
    if n >= 41:  # eigenvalue 1 of multiplicity 40 next to distinct ones
        w = np.concatenate([np.ones(40), np.linspace(-2.0, 0.8, (n - 40) // 2), np.linspace(1.2, 3.0, n - 40 - (n - 40) // 2)])
        A, V = ref.with_spectrum(w, rng)
        o = np.argsort(w, kind="stable")
        Vs = V[:, o]
        i0 = int(np.searchsorted(w[o], 1.0))
        out.append(("mult40", A, w[o], (Vs, [(list(range(i0, i0 + 40)), 0.2)])))
    if n >= 21:  # 20 eigenvalues within 1e-12 (relative) of each other
        w = np.concatenate([1.0 + 1e-12 * np.linspace(0.0, 1.0, 20), np.linspace(-2.0, 0.5, (n - 20) // 2),
                            np.linspace(1.5, 3.0, n - 20 - (n - 20) // 2)])
        A, V = ref.with_spectrum(w, rng)
        o = np.argsort(w, kind="stable")
        i0 = int(np.searchsorted(w[o], 1.0))
        out.append(("cluster20", A, w[o], (V[:, o], [(list(range(i0, i0 + 20)), 0.5)])))
    return out


def test_eigh_known_spectra_at_size_edges():
    """Every spectrum kind at sizes on both sides of 96 (QR_SMALL) and 128 (NB), all in ONE ragged batch (ldn 264)."""
    rng = np.random.default_rng(2024)
    cases = []
    for n in SIZES:
        cases += [(n,) + c for c in _spectrum_cases(n, rng)]
    lam, Q = _eigh([c[2] for c in cases], 264)
    for s, (n, kind, A, w, vec) in enumerate(cases):
        _check_eig(A, w, lam[s], Q[s], (n, kind), vec)


def test_eigh_ragged_abi_batch_with_nan_padding():
    """n = [0, 1, 97, 40, 129] at ldn = 160: an empty matrix, a 1 x 1, a cluster across the 96-row switch, glued Wilkinson matrices
    (near-degenerate pairs; mpmath spectrum) and a graded semi-definite one past a panel edge."""
    rng = np.random.default_rng(5)
    w97 = np.concatenate([1.0 + 1e-12 * np.linspace(0, 1, 20), np.linspace(-4.0, 0.0, 77)])
    A97, _ = ref.with_spectrum(w97, rng)
    A40 = ref.glued_wilkinson([21, 19], 1e-8)
    g = np.sort(10.0 ** (-17.0 * rng.uniform(0, 1, 129)))
    g[-1] = 1.0
    A129, _ = ref.with_spectrum(g, rng)
    mats = [np.zeros((0, 0)), np.array([[-3.5]]), A97, A40, A129]
    want = [np.zeros(0), np.array([-3.5]), np.sort(w97), ref.mp_eigvalsh(A40), g]
    lam, Q = _eigh(mats, 160)
    for s, (A, w) in enumerate(zip(mats, want)):
        _check_eig(A, w, lam[s], Q[s], ("ragged", A.shape[0]))


def test_eigh_wilkinson_vs_mpmath():
    """Wilkinson W21+ (pairs agreeing to 1e-14) and glued Wilkinson matrices, tridiagonal and densified by exact reflectors,
    against mpmath.eigsy at 30 digits."""
    rng = np.random.default_rng(9)
    tri = [ref.wilkinson_plus(21), ref.glued_wilkinson([13, 13, 13], 1e-12), ref.glued_wilkinson([21, 19], 1e-6)]
    want = [ref.mp_eigvalsh(A) for A in tri]
    mats, ws = list(tri), list(want)
    for A, w in zip(tri, want):  # the same spectra as dense matrices (V W V^T, V exactly orthogonal: its rounding moves them by < n eps)
        n = A.shape[0]
        M = np.asarray(A, dtype=ref.LD)
        for v in ref.reflectors(n, 4, rng):
            u = v.astype(ref.LD)
            c = ref.LD(2) / (u @ u)
            M = M - np.outer(u, c * (u @ M))
            M = M - np.outer(M @ u, c * u)
        mats.append((0.5 * (M + M.T)).astype(np.float64))
        ws.append(w)
    lam, Q = _eigh(mats, 48)
    for s, (A, w) in enumerate(zip(mats, ws)):
        _check_eig(A, w, lam[s], Q[s], ("wilkinson", s))


def test_eigh_batch_larger_than_a_repair_group():
    """33 matrices of 33 different n (one more than REPAIR_GROUP) in one call, sizes 0..200 across two panels."""
    rng = np.random.default_rng(33)
    ns = rng.choice(np.arange(2, 201), 33, replace=False)
    ns[0], ns[1], ns[2] = 0, 1, 96
    mats, ws = [], []
    for n in ns:
        w = np.sort(rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3))
        A, _ = ref.with_spectrum(w, rng) if n else (np.zeros((0, 0)), None)
        mats.append(A)
        ws.append(w)
    lam, Q = _eigh(mats, 200)
    for s, (A, w) in enumerate(zip(mats, ws)):
        _check_eig(A, w, lam[s], Q[s], ("batch33", A.shape[0]))


# ------------------------------------------------------------------------------------------------ imcom_solve_chol
C_CHOL = 50  # every Cholesky bound below: (base + c cond eps), cond = cond_2(A + kappa I)
TILE_NS = (1, 2, 16, 17, 127, 128, 129, 255, 256, 257)


def _solve_chol(As, mBs, Cs, kC, ldn, ucmin=1e-6, smax=0.5):
    """imcom_solve_chol on a ragged batch, A and -B/2 padded with NaN to ldn; outputs pre-filled with SENT."""
    lib, ctx, host = _lib()
    batch, m = len(As), mBs[0].shape[0]
    ns = np.array([a.shape[0] for a in As], np.int32)
    A = np.full((batch, ldn, ldn), np.nan)
    B = np.full((batch, m, ldn), np.nan)
    for s, (a, b) in enumerate(zip(As, mBs)):
        A[s, : a.shape[0], : a.shape[0]] = a
        B[s, :, : a.shape[0]] = b
    A0, B0 = A.copy(), B.copy()
    kC = np.ascontiguousarray(kC, dtype=np.float64)
    Cs = np.ascontiguousarray(Cs, dtype=np.float64)
    T = np.full((batch, m, ldn), SENT, np.float32)
    UC, Sg, kp = (np.full((batch, m), SENT, np.float32) for _ in range(3))
    info = np.full(batch, -7, np.int32)
    _check(lib.imcom_solve_chol(ctx, batch, _p(ns), ldn, m, _p(A), _p(B), _p(Cs), _p(kC), kC.size, ucmin, smax, _p(T), _p(UC),
                                _p(Sg), _p(kp), _p(info), host))
    assert np.array_equal(A, A0, equal_nan=True) and np.array_equal(B, B0, equal_nan=True)
    assert np.isfinite(T).all() and np.isfinite(UC).all() and np.isfinite(Sg).all() and np.isfinite(kp).all()
    return T, UC, Sg, kp, info


def _systems(ns, m, rng, spacing=0.75):
    """Gaussian-overlap systems (exp(-r^2/3), the form of test_chol_ragged_batch_vs_oracle) with a point density that makes A
    numerically semi-definite from a few dozen points on; C = A's scale."""
    out = []
    for n in ns:
        scale = float(rng.uniform(0.8, 1.3))
        A, mb = ref.gaussian_overlap(n, rng, width=max(1.0, spacing * np.sqrt(n)), scale=scale)
        out.append((A, mb(m), scale))
    return out


@pytest.mark.parametrize("m", [1, 17, 128])
@pytest.mark.parametrize("cond", [1e3, 1e8, 1e11])
def test_chol_tile_edges_vs_refined_solve(m, cond):
    """One kappa node, n on both sides of every tile edge up to 257 in one ragged batch (ldn 264 > max n, m > n for the small
    stamps), kappa chosen so that cond(A + kappa I) ~ `cond` where A allows it; against a float64 solve refined in long double."""
    rng = np.random.default_rng(int(np.log10(cond)) * 1000 + m)
    sys_ = _systems(TILE_NS, m, rng)
    # one kappa/C for the batch: lambda_max / C of the largest stamp over the target condition number
    big = sys_[-1]
    kC = np.linalg.eigvalsh(big[0])[-1] / big[2] / cond
    _chol_vs_refined(sys_, kC, 264)


def test_chol_many_output_pixels_and_ldn_equal_n():
    """m = 2500 (paper 3's n2f = 50), ldn = n for the largest stamp, cond ~ 1e11."""
    rng = np.random.default_rng(2500)
    sys_ = _systems((257, 16, 129), 2500, rng)
    kC = np.linalg.eigvalsh(sys_[0][0])[-1] / sys_[0][2] / 1e11
    _chol_vs_refined(sys_, kC, 257)


def _chol_vs_refined(sys_, kC, ldn):
    As, mBs, Cs = [s[0] for s in sys_], [s[1] for s in sys_], [s[2] for s in sys_]
    T, UC, Sg, kp, info = _solve_chol(As, mBs, Cs, [kC], ldn)
    for s, (A, mB, Cc) in enumerate(sys_):
        n = A.shape[0]
        kap = kC * Cc
        cond = ref.cond_spd(A, kap)
        Tr, Ur, Sr, scale = ref.chol_maps_refined(A, mB, Cc, kC)
        Tr = Tr.astype(np.float64)
        tag = (n, f"cond {cond:.1e}")
        assert info[s] == 0, tag
        assert np.all(T[s, :, n:] == 0), tag
        err = np.abs(T[s, :, :n] - Tr).max() / np.abs(Tr).max()
        assert err <= 1e-6 + C_CHOL * cond * EPS, (tag, err)
        tc = C_CHOL * cond * EPS
        # UC = 1 - (kappa N + D) / C is a difference of terms of size `scale` (~1): its error follows them, not UC
        assert np.all(np.abs(UC[s] - Ur) <= ATOL_MAP + (RTOL_MAP + tc) * np.maximum(np.abs(Ur), scale)), (tag, np.abs(UC[s] - Ur).max())
        assert np.allclose(Sg[s], Sr, rtol=RTOL_MAP + tc, atol=ATOL_MAP), tag
        assert np.allclose(kp[s], kap, rtol=1e-6, atol=0), tag


@pytest.mark.parametrize("nv", [1, 2, 4, 8])
def test_chol_kappa_nodes_vs_oracle(nv):
    """nv = 1, 2, 4, 8 ascending kappa nodes (8 = CHOL_MAXNV, the register-array bound of the multi-kappa kernels) on a ragged
    batch across tile edges, against oracle.chol_kernel (lakernel.CholKernel with build_reduced_T_wrap)."""
    from oracle import oracle as orc

    rng = np.random.default_rng(80 + nv)
    # (n >= 127: with 8 nodes on 17 pixels the reference's own reduced system (build_reduced_T_wrap) is singular -- NaN maps)
    sys_ = _systems((127, 128, 129, 256, 257), 128, rng)
    kC = np.array([3e-4]) if nv == 1 else np.logspace(-6, -2, nv)
    T, UC, Sg, kp, info = _solve_chol([s[0] for s in sys_], [s[1] for s in sys_], [s[2] for s in sys_], kC, 260)
    for s, (A, mB, Cc) in enumerate(sys_):
        n = A.shape[0]
        To, Uo, So, ko, info_o = orc.chol_kernel(A.copy(), mB.copy(), Cc, kC, 1e-6, 0.5)
        cond = ref.cond_spd(A, kC[0] * Cc)
        tc = C_CHOL * cond * EPS
        tag = (nv, n, f"cond {cond:.1e}")
        assert info[s] == 0 and info_o == 0, tag
        assert np.all(T[s, :, n:] == 0), tag
        assert np.abs(T[s, :, :n] - To).max() <= (1e-6 + tc) * np.abs(To).max(), tag
        assert np.allclose(UC[s], Uo, rtol=RTOL_MAP + tc, atol=ATOL_MAP), (tag, np.abs(UC[s] - Uo).max())
        assert np.allclose(Sg[s], So, rtol=RTOL_MAP + tc, atol=ATOL_MAP), tag
        assert np.allclose(kp[s], ko, rtol=1e-5, atol=0), tag


def test_chol_more_kappa_nodes_than_supported_is_refused():
    """nv = 9 > CHOL_MAXNV: an argument error with a message, before anything is launched or written; the context stays usable."""
    from oracle import oracle as orc

    lib, ctx, host = _lib()
    rng = np.random.default_rng(9)
    (A, mB, Cc), = _systems((20,), 4, rng)
    n, m = 20, 4
    ns = np.array([n], np.int32)
    Cs = np.array([Cc])
    T = np.full((1, m, n), SENT, np.float32)
    UC, Sg, kp = (np.full((1, m), SENT, np.float32) for _ in range(3))
    info = np.full(1, -7, np.int32)
    args = lambda kC: (ctx, 1, _p(ns), n, m, _p(A), _p(mB), _p(Cs), _p(kC), kC.size, 1e-6, 0.5, _p(T), _p(UC), _p(Sg), _p(kp), _p(info), host)
    kC9 = np.logspace(-6, -2, 9)
    status = lib.imcom_solve_chol(*args(kC9))
    assert status != 0
    assert "nv=9" in lib.imcom_last_error().decode()
    assert np.all(T == SENT) and np.all(UC == SENT) and info[0] == -7
    kC3 = np.ascontiguousarray(kC9[::4])  # (8 nodes on 20 pixels would make the reference's own reduced system singular)
    _check(lib.imcom_solve_chol(*args(kC3)))
    To, Uo, So, ko, info_o = orc.chol_kernel(A.copy(), mB.copy(), Cc, kC3, 1e-6, 0.5)
    assert np.isfinite(To).all() and np.isfinite(Uo).all()
    tc = C_CHOL * ref.cond_spd(A, kC3[0] * Cc) * EPS
    assert info[0] == info_o == 0
    assert np.abs(T[0] - To).max() <= (1e-6 + tc) * np.abs(To).max()
    assert np.allclose(UC[0], Uo, rtol=RTOL_MAP + tc, atol=ATOL_MAP) and np.allclose(Sg[0], So, rtol=RTOL_MAP + tc, atol=ATOL_MAP)


# ------------------------------------------------------------------------------------------------ the two repair paths
def test_chol_repair_on_both_sides_of_the_subspace_switch(monkeypatch):
    """Stamps of n = 1000, 1023 (w[0] from the eigensolver) and 1024, 1100 (from the 16-vector subspace iteration) in ONE batch
    (padded to 1152), made indefinite by A - c kappa I with different c so that w[0] lies in the dense low end of the spectrum, next
    to a healthy stamp; then again with IMCOM_LMIN=eigh, which sends every repair to the eigensolver."""
    from oracle import oracle as orc
    from pyimcom_amd._lib import default_context

    rng = np.random.default_rng(1152)
    ns = (1000, 1023, 1024, 1100, 700)
    c_shift = (3.0, 1.5, 40.0, 8.0, 0.0)
    kC = np.array([2e-4])
    m = 64
    sys_, want = [], []
    for n, c in zip(ns, c_shift):
        (A, mB, Cc), = _systems((n,), m, rng, spacing=0.5)
        A = A - c * kC[0] * Cc * np.eye(n)
        sys_.append((A, mB, Cc))
        want.append(orc.chol_kernel(A.copy(), mB.copy(), Cc, kC, 1e-6, 0.5) + (np.linalg.eigvalsh(A),))
    w0_true = [w[5][0] for w, c in zip(want, c_shift) if c]
    assert all(w < -kC[0] * 0.5 for w in w0_true)  # (every shifted stamp is indefinite beyond kappa)
    ctx = default_context()
    runs = {}
    for mode in ("default", "eigh"):
        if mode == "eigh":
            monkeypatch.setenv("IMCOM_LMIN", "eigh")
        T, UC, Sg, kp, info = _solve_chol([s[0] for s in sys_], [s[1] for s in sys_], [s[2] for s in sys_], kC, 1100)
        cnt, lo, hi = ctx.last_repair()
        assert cnt == 4, (mode, cnt)
        assert abs(lo - min(w0_true)) <= 1e-9 * abs(min(w0_true)), (mode, lo, min(w0_true))
        assert abs(hi - max(w0_true)) <= 1e-9 * abs(max(w0_true)), (mode, hi, max(w0_true))
        runs[mode] = T
        for s, (A, mB, Cc) in enumerate(sys_):
            To, Uo, So, ko, info_o, lam = want[s]
            n, kap = A.shape[0], kC[0] * Cc
            tag = (mode, n)
            assert int(info[s]) == info_o == (1 if c_shift[s] else 0), tag
            # after the repair the smallest eigenvalue of the factored matrix is kappa + 1e-16 (tests/test_gpu_stamps.py)
            cond = (lam[-1] + kap + abs(min(lam[0], 0.0))) / kap
            tc = C_CHOL * cond * EPS
            assert np.all(T[s, :, n:] == 0), tag
            assert np.abs(T[s, :, :n] - To).max() <= (1e-6 + tc) * np.abs(To).max(), tag
            assert np.allclose(UC[s], Uo, rtol=RTOL_MAP + tc, atol=ATOL_MAP), tag
            assert np.allclose(Sg[s], So, rtol=RTOL_MAP + tc, atol=ATOL_MAP), tag
            assert np.allclose(kp[s], ko, rtol=1e-5, atol=0), tag
    for s, (A, _, Cc) in enumerate(sys_):  # the two ways to w[0] agree
        n, lam = A.shape[0], want[s][5]
        kap = kC[0] * Cc
        cond = (lam[-1] + kap + abs(min(lam[0], 0.0))) / kap
        a, b = runs["default"][s, :, :n], runs["eigh"][s, :, :n]
        assert np.abs(a - b).max() <= (1e-6 + C_CHOL * cond * EPS) * np.abs(b).max(), n
