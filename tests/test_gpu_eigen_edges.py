"""The Eigen kernel's solve (imcom_solve_eigen / imcom_solve_eigen_resident, csrc/eigen.hip) in BOTH bases -- the band basis and
the tridiagonal one (IMCOM_EIGEN_BASIS=tridiagonal; by itself above 4.8k rows) -- at its size and search edges: stamp sizes around
the four-row phase groups and the 128-row reflector panels, output-pixel counts around the 64-lane workgroups, 0, 1 and 13
bisection steps, a search that sigma_max decides, the chunked band solve with four chunks, the resident entry and the
eigendecomposition fallback among positive definite neighbours.  Against tests/eigen_reference.py: the maps at the device's own
kappa from a solve refined in long double, and every bisection decision judged one by one along the device's path (statements
(a) to (c) there).  Direct C-ABI calls; the padding of every host input is NaN and must not reach an output."""

import ctypes as C

import numpy as np
import pytest

from tests import eigen_reference as er

pytestmark = pytest.mark.gpu

SENT = 7.0  # outputs are pre-filled with this: what the library must overwrite (or zero) is seen to be written


@pytest.fixture(params=["band", "tridiagonal"])
def basis(request, monkeypatch):
    """The variable is read at every call (csrc/eigen.hip eigen_uses_band)."""
    if request.param == "tridiagonal":
        monkeypatch.setenv("IMCOM_EIGEN_BASIS", "tridiagonal")
    else:
        monkeypatch.delenv("IMCOM_EIGEN_BASIS", raising=False)
    return request.param


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _solve(case, ldn, kC=None):
    """imcom_solve_eigen on the case's ragged batch, A and -B/2 padded with NaN to ldn; outputs pre-filled with SENT."""
    from pyimcom_amd._lib import MEM_HOST, check, default_context, lib

    batch, m = len(case.stamps), case.m
    ns = np.array([st.n for st in case.stamps], np.int32)
    A = np.full((batch, ldn, ldn), np.nan)
    B = np.full((batch, m, ldn), np.nan)
    for s, st in enumerate(case.stamps):
        A[s, : st.n, : st.n] = st.A
        B[s, :, : st.n] = st.mB
    A0, B0 = A.copy(), B.copy()
    Cs = np.array([st.C for st in case.stamps])
    kC = np.ascontiguousarray(case.kC if kC is None else kC, dtype=np.float64)
    T = np.full((batch, m, ldn), SENT, np.float32)
    UC, Sg, kp = (np.full((batch, m), SENT, np.float32) for _ in range(3))
    info = np.full(batch, -7, np.int32)
    check(lib.imcom_solve_eigen(default_context().handle, batch, _p(ns), ldn, m, _p(A), _p(B), _p(Cs), _p(kC), kC.size, float(case.target),
                                float(case.smax), int(case.nbis), _p(T), _p(UC), _p(Sg), _p(kp), _p(info), MEM_HOST))
    assert np.array_equal(A, A0, equal_nan=True) and np.array_equal(B, B0, equal_nan=True)  # the inputs are not modified
    assert np.isfinite(T).all() and np.isfinite(UC).all() and np.isfinite(Sg).all() and np.isfinite(kp).all()
    return T, UC, Sg, kp, info


def _judge(case, out, basis):
    """info, the zero columns of T, the empty stamps, and statements (a) to (c) for every stamp; the share of pixels that hold a
    within-bound decision.  Returns s_alone [batch][m] of the replay (where sigma_max alone sent kappa up)."""
    T, UC, Sg, kp, info = out
    want = case.info if case.info is not None else [0] * len(case.stamps)
    assert info.tolist() == want, info
    tied, dmap, ddec = 0, 0.0, 0.0
    s_alone = np.zeros((len(case.stamps), case.m), bool)
    for s, st in enumerate(case.stamps):
        n = st.n
        tag = (case.name, basis, "stamp", s, "n", n)
        assert np.all(T[s, :, n:] == 0), tag
        if n == 0:
            assert np.all(UC[s] == 1) and np.all(Sg[s] == 0) and np.all(kp[s] == 1), tag  # lakernel.py:110-119
            continue
        r = er.check_stamp(case, st, T[s, :, :n], UC[s], Sg[s], kp[s], tag)
        tied += r["tied"]
        s_alone[s] = r["s_alone"]
        dmap, ddec = max(dmap, r["dist_map"]), max(ddec, r["dist_dec"])
    print(f"[eigen edges] {case.name} ({basis}): maps {dmap:.3f} cond eps beyond their float32 base, decisions against the reference "
          f"up to margin {ddec:.3f} max(n,8) eps cond, {tied} pixels with a within-bound decision")
    assert tied <= er.MAX_TIED * len(case.stamps) * case.m, tied
    return s_alone


# ------------------------------------------------------------------------------------------------ 1, 2: size edges
@pytest.mark.parametrize("m", [1, 63, 64, 65])
@pytest.mark.parametrize("cond", [1e3, 1e8, 1e11])
def test_size_edges_single_kappa(basis, m, cond):
    """n = 0..9 (the four-row phase groups), 16, 17, and both sides of 128 and 256 (the reflector panels) in ONE ragged batch
    (ldn 264), m on both sides of a 64-lane workgroup, kappa such that cond(A + kappa I) ~ `cond` for the largest stamps."""
    case = er.size_case(m, cond)
    _judge(case, _solve(case, 264), basis)


@pytest.mark.parametrize("m", [1, 63, 64, 65])
@pytest.mark.parametrize("q", [0.3, 0.7])
def test_size_edges_search(basis, m, q):
    """The same batch searched (13 steps, cond 1e3 at kappa_min, bracket 1e4), the target between two neighbouring UC values at
    mid-bracket; and the same call with five nodes between the same ends gives the same bits: interior nodes do not matter."""
    case = er.search_case(m, q)
    out = _solve(case, 264)
    _judge(case, out, basis)
    kC5 = np.array([case.kC[0], 1.7 * case.kC[0], 40.0 * case.kC[0], 0.6 * case.kC[1], case.kC[1]])
    for a, b in zip(out, _solve(case, 264, kC5)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("nbis", [0, 1])
def test_no_and_one_bisection_step(basis, nbis):
    """nbis = 0: every kappa is sqrt(kmin kmax) (times C); nbis = 1: one of its two neighbours; the maps at that kappa."""
    case = er.search_case(65, 0.3, nbis)
    out = _solve(case, 264)
    _judge(case, out, basis)
    steps = []
    for s, st in enumerate(case.stamps):
        if st.n:
            kmin, kmax = case.ends(st)  # (the reported kappa is the bisection's times C once more: lakernel.py:222)
            steps.append(np.log(out[3][s].astype(np.float64) / st.C / np.sqrt(kmin * kmax)) / er.grid_step(kmin, kmax, nbis))
    steps = np.concatenate(steps)
    assert np.all(np.abs(np.abs(steps) - nbis) < 1e-3), steps
    assert nbis == 0 or (steps.min() < 0 < steps.max())  # the one decision goes both ways within the batch


def test_sigma_max_decides(basis):
    """sigma_max between two neighbouring S at mid-bracket and the target below every UC: the S < smax half of the decision alone
    sends kappa up, at some step of at least a third of the pixels."""
    case = er.smax_case()
    s_alone = _judge(case, _solve(case, 264), basis)
    live = sum(st.n > 0 for st in case.stamps) * case.m
    assert s_alone.sum() >= live / 3, (int(s_alone.sum()), live)


# ------------------------------------------------------------------------------------------------ 5: the chunked band solve
@pytest.mark.parametrize("search", [False, True], ids=["single", "search"])
@pytest.mark.parametrize("batch,split", [(130, None), (65, "1")])
def test_chunked_band_solve(basis, batch, split, search, monkeypatch):
    """130 stamps (five systems of n <= 128 repeated, n = 0 and 1 among them) with m = 200: mp = 256 and, in the band basis, FOUR
    launches of band_solve_kernel of 64 columns each for a sub-batch above 64 stamps -- a0 > 0, the last chunk with 8 live columns,
    the factors indexed by the column within the chunk.  The default split makes two sub-batches of 65; IMCOM_EIGEN_SPLIT=1 with 65
    stamps one.  In the tridiagonal basis the same shapes are simply a large batch."""
    if split:
        monkeypatch.setenv("IMCOM_EIGEN_SPLIT", split)
    else:
        monkeypatch.delenv("IMCOM_EIGEN_SPLIT", raising=False)
    case = er.chunk_case(batch, search)
    _judge(case, _solve(case, 128), basis)


# ------------------------------------------------------------------------------------------------ 6: the resident entry
@pytest.mark.parametrize("search", [False, True], ids=["single", "search"])
@pytest.mark.parametrize("m,ldm", [(65, 128), (200, 256)])
def test_resident_entry(basis, m, ldm, search):
    """imcom_solve_eigen_resident on device tensors, ldn = 384: A with the identity in its padding and Bt zero-padded, as
    imcom_build_A / imcom_build_B leave them; Tt zero in rows >= n and columns >= m."""
    import torch

    from pyimcom_amd._dev import bound_context
    from pyimcom_amd._lib import check, lib, ptr

    case = er.resident_case(m, search)
    batch, ldn = len(case.stamps), 384
    ns = np.array([st.n for st in case.stamps], np.int32)
    A = np.zeros((batch, ldn, ldn))
    Bt = np.zeros((batch, ldn, ldm))
    for s, st in enumerate(case.stamps):
        A[s, : st.n, : st.n] = st.A
        A[s, np.arange(st.n, ldn), np.arange(st.n, ldn)] = 1.0
        Bt[s, : st.n, :m] = st.mB.T
    dev = torch.device("cuda:0")
    A_d, Bt_d = torch.from_numpy(A).to(dev), torch.from_numpy(Bt).to(dev)
    Tt = torch.full((batch, ldn, ldm), SENT, dtype=torch.float32, device=dev)
    UC, Sg, kp = (torch.full((batch, m), SENT, dtype=torch.float32, device=dev) for _ in range(3))
    Cs = np.array([st.C for st in case.stamps])
    kC = np.ascontiguousarray(case.kC)
    info = np.full(batch, -7, np.int32)
    ctx = bound_context(dev)
    check(lib.imcom_solve_eigen_resident(ctx.handle, batch, _p(ns), ldn, m, ldm, ptr(A_d), ptr(Bt_d), _p(Cs), _p(kC), kC.size, float(case.target),
                                         float(case.smax), int(case.nbis), ptr(Tt), ptr(UC), ptr(Sg), ptr(kp), _p(info)))
    torch.cuda.synchronize()
    assert np.array_equal(A_d.cpu().numpy(), A) and np.array_equal(Bt_d.cpu().numpy(), Bt)
    Tt = Tt.cpu().numpy()
    assert np.isfinite(Tt).all()
    for s, st in enumerate(case.stamps):
        assert np.all(Tt[s, st.n:, :] == 0) and np.all(Tt[s, :, m:] == 0), s
    T = np.ascontiguousarray(Tt[:, :, :m].transpose(0, 2, 1))  # [batch][m][ldn]
    _judge(case, (T, UC.cpu().numpy(), Sg.cpu().numpy(), kp.cpu().numpy(), info), basis)


# ------------------------------------------------------------------------------------------------ 7: the fallback among the edges
@pytest.mark.parametrize("search", [False, True], ids=["single", "search"])
def test_indefinite_stamps_among_positive_definite_neighbours(basis, search):
    """Stamps of n = 2, 5, 129 with eigenvalues in [-2, -1] and [1, 2] (A + kappa I indefinite and well conditioned over the whole
    bracket) between positive definite stamps and an empty one: info = 1 exactly on them, their results against the LU-refined
    reference with the same statements, and the neighbours bit-identical to the same call without the indefinite stamps."""
    case = er.indef_case(search)
    assert sum(case.info) == 3
    out = _solve(case, 136)
    _judge(case, out, basis)
    alone = er.indef_case(search, False)
    out_alone = _solve(alone, 136)
    assert out_alone[4].tolist() == [0] * len(alone.stamps)
    keep = [s for s in range(len(case.stamps)) if s not in er.INDEF_AT]
    for a, b in zip(out, out_alone):
        assert np.array_equal(a[keep], b)
