"""Reference of the Eigen kernel's edge tests (tests/test_gpu_eigen_edges.py; checked itself by tests/test_eigen_reference.py).

The Eigen kernel (csrc/eigen.hip; lakernel.EigenKernel, lakernel.py:141-223) gives, per output pixel with right-hand side b and
per-pixel kappa,  x = (A + kappa I)^-1 b,  D = b^T x,  S = x^T x (Sigma),  UC = 1 - (D + kappa S) / C,  and with several kappa
nodes it first bisects kappa per pixel (routine.lakernel1): nbis steps from sqrt(kmin kmax), each one DOWN by the current factor
where  udc > target and S < smax,  else UP.  Numpy and scipy only:

  maps_at   the maps at given kappa from a float64 factorisation refined with long-double residuals (la_reference.solve_refined,
            its LU twin where A + kappa I is indefinite): the yardstick of every number.
  sums      the reference's own eigen-sums in long double from a float64 eigh: used only to replay decisions; the CPU test bounds its
            distance from maps_at.
  replay    the device's kappa decoded into its decision sequence and judged step by step ALONG THE DEVICE'S PATH.

The parity statement, per pixel of a multi-kappa call: (a) kappa decodes to a node of the bisection grid; (b) every decision on the
device's path equals the reference decision at that step unless the reference's margin there is below
C_DEC max(n, 8) eps cond(A + kmin I); (c) T, UC, Sigma equal maps_at AT THE DEVICE'S OWN kappa within base + C_MAP cond eps of
their scales.  No pixel is excluded and no flip allowed; at most 2 % of a case's pixels may hold a within-bound decision
(MAX_TIED), which the CPU test asserts for the reference's own path on every committed case.

Constants (the project's 10 ref_err convention; `python -m tests.eigen_reference` prints the measurements):
  the float64 oracle (numpy eigh + the C lakernel1 of oracle/, a backward-stable float64 method of the same conditioning) lies at
  most ORACLE_MAP = 3.0 cond eps from maps_at over T, UC and Sigma of the committed single-kappa and search cases, and at most
  ORACLE_DEC = 0.38 max(n, 8) eps cond(A + kmin I) over udc and S at mid-bracket and at the final kappa of the search cases;
  C_MAP = 10 ORACLE_MAP = 30, C_DEC = 10 ORACLE_DEC = 3.8.  The indefinite stamps (another route on the device, the LU reference,
  cond ~ 3 so that cond eps no longer hides the oracle's n eps) are measured on their own: 11.7 cond eps and 9.73 max(n, 8) eps cond;
  C_MAP_INDEF = 117, C_DEC_INDEF = 97.3.
  Device (MI355X, both bases, every committed case): T, UC and Sigma lie at most 0.21 cond eps from maps_at beyond their float32
  store (seen at cond 1e11 only; below the float32 resolution of the outputs elsewhere); every kappa decoded to a node and NO decision
  of any pixel differed from the reference's, so no pixel held a within-bound decision (distance 0 of the C_DEC = 3.8 allowed)."""

import functools
from dataclasses import dataclass, field

import numpy as np

from tests.la_reference import EPS, LD, gaussian_overlap, solve_refined, solve_refined_lu, with_spectrum

ORACLE_MAP, ORACLE_DEC = 3.0, 0.38  # measured: see the docstring
C_MAP, C_DEC = 10 * ORACLE_MAP, 10 * ORACLE_DEC
ORACLE_MAP_INDEF, ORACLE_DEC_INDEF = 11.7, 9.73
C_MAP_INDEF, C_DEC_INDEF = 10 * ORACLE_MAP_INDEF, 10 * ORACLE_DEC_INDEF

MAX_TIED = 0.02  # share of a case's pixels that may hold a decision within the bound
F32 = 2.0 ** -24  # half a float32 ulp, relative
EDGE_NS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 127, 128, 129, 255, 256, 257)
NO_SMAX = 1e30
RTOL_MAP, ATOL_MAP = 1e-5, 1e-9  # UC, Sigma (tests/test_gpu_la_edges.py)


# ------------------------------------------------------------------------------------------------ the maps at given kappa
def maps_at(A, b, C, kappa):
    """b [m][n], kappa scalar or [m] (absolute, not over C).  One refined solve (one factorisation) per distinct kappa.
    Returns T [m][n] (long double), UC, S, scale = (kappa S + |D|) / C of the two terms whose difference UC is (float64)."""
    m, n = b.shape
    kap = np.broadcast_to(np.asarray(kappa, dtype=np.float64), (m,))
    T = np.zeros((m, n), dtype=LD)
    for k in np.unique(kap):
        sel = np.flatnonzero(kap == k)
        try:
            X = solve_refined(A, float(k), b[sel].T)
        except np.linalg.LinAlgError:
            X = solve_refined_lu(A, float(k), b[sel].T)
        T[sel] = X.T
    D = np.einsum("ai,ai->a", b.astype(LD), T)
    S = np.einsum("ai,ai->a", T, T)
    kl = kap.astype(LD)
    UC = 1 - (D + kl * S) / LD(C)
    return T, UC.astype(np.float64), S.astype(np.float64), ((kl * S + np.abs(D)) / LD(C)).astype(np.float64)


def sums(lam, P, C, kappa):
    """The reference's sums (routine.py:405-419) in long double: lam [n] and P = b Q [m][n] from a float64 eigh, kappa [m].
    Returns S = sum P^2 / (lam + kappa)^2, udc = 1 - sum (lam + 2 kappa) P^2 / (lam + kappa)^2 / C and the scale of udc's terms."""
    l, k = lam.astype(LD)[None, :], np.asarray(kappa, dtype=LD)[:, None]
    v2 = (P.astype(LD) / (l + k)) ** 2
    S = v2.sum(1)
    s1 = ((l + 2 * k) * v2).sum(1)
    return S, 1 - s1 / LD(C), (np.abs(((l + k) * v2).sum(1)) + k[:, 0] * S) / LD(C)


# ------------------------------------------------------------------------------------------------ the bisection grid
def grid_step(kmin, kmax, nbis):
    """ln r of the grid after nbis steps: kappa = sqrt(kmin kmax) r^j, j odd (j = 0 for nbis = 0), |j| < 2^nbis."""
    return float(np.log(kmax / kmin)) / 2.0 ** (nbis + 1)


def decode(kappa_dev, C, kmin, kmax, nbis):
    """The device's kappa [m] (float32: the bisection's kappa stored as float32 and THEN multiplied by C, lakernel.py:216-222;
    kmin, kmax are the absolute ends kappaC C) -> (ok [m], up [m][nbis]): ok where kappa is a node of the grid to within the two
    float32 roundings, up[a][it] = step `it` multiplied kappa by the factor (the decision was False)."""
    k = np.asarray(kappa_dev, dtype=np.float64) / C  # undo the quirk
    lnr = grid_step(kmin, kmax, nbis)
    with np.errstate(all="ignore"):
        x = (np.log(k) - 0.5 * np.log(kmin * kmax)) / lnr
    fin = np.isfinite(x)  # (NaN, zero and negative kappa are no nodes)
    x = np.where(fin, x, 0.0)
    j = np.rint(x)
    ok = fin & (np.abs(x - j) * lnr <= 4 * F32)  # store, product, and the float64 noise of the device's sqrt chain
    if nbis == 0:
        return ok & (j == 0), np.zeros((k.size, 0), bool)
    ok &= (np.abs(j) < 2.0 ** nbis) & (np.mod(j, 2) == 1)
    code = ((np.where(ok, j, 1) + 2.0 ** nbis - 1) / 2).astype(np.int64)  # j = sum (+-1) 2^(nbis-1-it): its binary digits, first step first
    up = (code[:, None] >> (nbis - 1 - np.arange(nbis))[None, :]) & 1
    return ok, up.astype(bool)


def path(up, kmin, kmax):
    """kappa [m][nbis + 1] visited by the decisions up [m][nbis] (long double): column `it` is where step `it` is decided, the last
    column the final kappa."""
    m, nbis = up.shape
    lnr = np.log(LD(kmax) / LD(kmin)) / LD(2.0) ** (nbis + 1)
    j = np.zeros((m, nbis + 1), dtype=LD)
    for it in range(nbis):
        j[:, it + 1] = j[:, it] + np.where(up[:, it], 1, -1) * LD(2.0) ** (nbis - 1 - it)
    return np.sqrt(LD(kmin) * LD(kmax)) * np.exp(j * lnr)


def _judge(S, udc, scale, target, smax):
    """Reference decision (udc > target) and (S < smax) with the margin of whichever comparison could change it: relative to the
    scale of udc's terms for udc, to S for S."""
    cu, cs = udc > target, S < smax
    mu, ms = np.abs(udc - target) / scale, np.abs(S - smax) / S
    dec = cu & cs
    # True: either comparison failing flips it; both False: both would have to change; else the one that is False
    margin = np.where(dec, np.minimum(mu, ms), np.where(~cu & ~cs, np.maximum(mu, ms), np.where(cu, ms, mu)))
    return dec, margin.astype(np.float64), cu & ~cs


def replay(lam, P, C, kmin, kmax, target, smax, nbis, kappa_dev):
    """Decode kappa_dev and walk the device's path in long double.  Returns (ok [m], dev [m][nbis], ref [m][nbis],
    margin [m][nbis], s_alone [m][nbis]): dev = the device's decision at each step (True = kappa went DOWN), ref = the reference
    decision at the same kappa, margin as in _judge, s_alone = udc > target held and S >= smax sent kappa up.  Rows of pixels that
    are not ok are meaningless."""
    ok, up = decode(kappa_dev, C, kmin, kmax, nbis)
    kp = path(up, kmin, kmax)
    m = up.shape[0]
    ref, margin, s_alone = (np.zeros((m, nbis), dt) for dt in (bool, np.float64, bool))
    for it in range(nbis):
        S, udc, scale = sums(lam, P, C, kp[:, it])
        ref[:, it], margin[:, it], s_alone[:, it] = _judge(S, udc, scale, target, smax)
    return ok, ~up, ref, margin, s_alone


def bisect(lam, P, C, kmin, kmax, target, smax, nbis):
    """The reference's own bisection in long double: (kappa [m] float64, margin [m][nbis])."""
    m = P.shape[0]
    up, margin = np.zeros((m, nbis), bool), np.zeros((m, nbis))
    for it in range(nbis):
        kp = path(up[:, :it], kmin, kmax)[:, -1] if it else np.full(m, np.sqrt(LD(kmin) * LD(kmax)))
        # (the grid of `it` steps is the grid of nbis steps at even j: the same kappa)
        S, udc, scale = sums(lam, P, C, kp)
        dec, margin[:, it], _ = _judge(S, udc, scale, target, smax)
        up[:, it] = ~dec
    return path(up, kmin, kmax)[:, -1].astype(np.float64), margin


def dec_bound(n, cond, indef=False):
    return (C_DEC_INDEF if indef else C_DEC) * max(n, 8) * EPS * cond


def cond_sym(lam, kappa):
    """2-norm condition number of A + kappa I of either sign, from A's eigenvalues."""
    a = np.abs(lam + kappa)
    return a.max() / a.min()


# ------------------------------------------------------------------------------------------------ cases
@dataclass(eq=False)
class Stamp:
    A: np.ndarray  # [n][n]
    mB: np.ndarray  # [m][n] = -B/2
    C: float
    _eig: tuple = field(default=None, repr=False)
    memo: dict = field(default_factory=dict, repr=False)  # references of this stamp by the kappa they were asked at

    @property
    def n(self):
        return self.A.shape[0]

    def eig(self):
        """(lam, P = mB Q) from numpy's float64 eigh, once."""
        if self._eig is None:
            lam, Q = np.linalg.eigh(self.A)
            self._eig = (lam, self.mB @ Q)
        return self._eig


@dataclass(eq=False)
class Case:
    name: str
    stamps: list
    kC: np.ndarray  # kappa / C nodes of the call (only the ends matter to the search)
    target: float = 1e-6
    smax: float = NO_SMAX
    nbis: int = 13
    info: list = None  # expected info vector (default: zeros)

    @property
    def m(self):
        return self.stamps[0].mB.shape[0]

    def ends(self, st):
        return self.kC[0] * st.C, self.kC[-1] * st.C


def systems(ns, m, rng, spacing=0.75):
    """Gaussian-overlap systems as tests/test_gpu_la_edges._systems: C = A's scale, drawn from [0.8, 1.3]."""
    out = []
    for n in ns:
        scale = float(rng.uniform(0.8, 1.3))
        A, mb = gaussian_overlap(n, rng, width=max(1.0, spacing * np.sqrt(n)), scale=scale)
        out.append(Stamp(A, mb(m), scale))
    return out


def bracket(stamps, cond=1e3, ratio=1e4):
    """kappa / C ends of a call: kmin = lambda_max / cond of the stamp with the largest lambda_max, kmax = ratio kmin."""
    k0 = max(st.eig()[0][-1] / st.C for st in stamps if st.n) / cond
    return np.array([k0, ratio * k0])


def _between(values, q):
    """Halfway between the two neighbouring sorted values at quantile q (never one of the values: they must differ)."""
    v = np.unique(values)
    i = min(max(int(q * (v.size - 1)), 0), v.size - 2)
    return 0.5 * (v[i] + v[i + 1])


def mid_maps(stamps, kC):
    """UC and S of every pixel of the non-empty stamps at mid-bracket (pooled)."""
    U, S = [], []
    for st in stamps:
        if st.n:
            _, u, s, _ = maps_at(st.A, st.mB, st.C, np.sqrt(kC[0] * kC[-1]) * st.C)
            U.append(u)
            S.append(s)
    return np.concatenate(U), np.concatenate(S)


@functools.lru_cache(maxsize=None)
def size_case(m, cond=1e3):
    """Single kappa on the ragged batch of every size edge."""
    rng = np.random.default_rng(int(np.log10(cond)) * 1000 + m)
    stamps = systems(EDGE_NS, m, rng)
    return Case(f"size m={m} cond={cond:.0e}", stamps, bracket(stamps, cond)[:1])


@functools.lru_cache(maxsize=None)
def search_case(m, q, nbis=13):
    """The same batch, searched: the leakage target between two neighbouring UC values at mid-bracket, at quantile q."""
    stamps = size_case(m).stamps
    kC = bracket(stamps)
    return Case(f"search m={m} q={q} nbis={nbis}", stamps, kC, _between(mid_maps(stamps, kC)[0], q), nbis=nbis)


@functools.lru_cache(maxsize=None)
def smax_case(m=65):
    """smax between two neighbouring S at mid-bracket (median), the target below every UC: only S < smax decides."""
    stamps = size_case(m).stamps
    kC = bracket(stamps)
    return Case(f"smax m={m}", stamps, kC, -1.0, _between(mid_maps(stamps, kC)[1], 0.5))


CHUNK_NS = (128, 0, 1, 77, 100)


@functools.lru_cache(maxsize=None)
def chunk_case(batch, search, m=200):
    """Five distinct systems with n <= 128 repeated to `batch` stamps, m = 200: mp = 256, four chunks of 64 columns in the band
    basis' solve for sub-batches above 64 stamps, the last chunk with 8 live columns."""
    rng = np.random.default_rng(200)
    five = systems(CHUNK_NS, m, rng)
    stamps = [five[s % 5] for s in range(batch)]  # (the same Stamp objects: their references are computed once)
    kC = bracket(five)
    if not search:
        return Case(f"chunk batch={batch} single", stamps, kC[:1])
    return Case(f"chunk batch={batch} search", stamps, kC, _between(mid_maps(five, kC)[0], 0.5))


RESIDENT_NS = (129, 0, 5, 256, 1, 257, 128)


@functools.lru_cache(maxsize=None)
def resident_case(m, search):
    rng = np.random.default_rng(384 + m)
    stamps = systems(RESIDENT_NS, m, rng)
    kC = bracket(stamps)
    if not search:
        return Case(f"resident m={m} single", stamps, kC[:1])
    return Case(f"resident m={m} search", stamps, kC, _between(mid_maps(stamps, kC)[0], 0.3))


INDEF_AT = {1: 2, 3: 5, 6: 129}  # position in the batch -> n of the indefinite stamps


@functools.lru_cache(maxsize=None)
def indef_case(search, with_indef=True, m=65):
    """Indefinite stamps (eigenvalues in [-2, -1] and [1, 2]: A + kappa I indefinite and well conditioned for the bracket inside
    [0.01, 0.1]) of n = 2, 5, 129 between positive definite neighbours and an empty stamp.  with_indef = False: the same call
    without them (the neighbours must not notice)."""
    rng = np.random.default_rng(7129)
    pd = systems((4, 17, 0, 130, 9), m, rng)  # (130: the padded size of the call is the same with and without the indefinite 129)
    for st in pd:  # eigenvalues of order one for every neighbour, so that the bracket suits all stamps
        if st.n:
            st.A = st.A + 0.5 * st.C * np.eye(st.n)
    stamps, it = [], iter(pd)
    for pos in range(len(pd) + len(INDEF_AT)):
        if pos in INDEF_AT:
            n = INDEF_AT[pos]
            w = np.concatenate([-rng.uniform(1, 2, n // 2), rng.uniform(1, 2, n - n // 2)])
            A, _ = with_spectrum(rng.permutation(w), rng)
            st = Stamp(A, rng.standard_normal((m, n)) * 0.3, float(rng.uniform(0.8, 1.3)))
            if with_indef:
                stamps.append(st)
        else:
            stamps.append(next(it))
    kC = np.array([0.02, 0.06])  # times C in [0.8, 1.3]: inside [0.01, 0.1]
    info = [int(st.n > 0 and st.eig()[0][0] < 0) for st in stamps]
    if not search:
        return Case(f"indef single {with_indef}", stamps, kC[:1], info=info)
    # Over so narrow a bracket UC hardly moves, and a target between two pixels sends every pixel straight to an end.  So the target is
    # the UC of one pixel of the indefinite n = 129 stamp at a kappa strictly inside the bracket and off the grid: that pixel homes in
    # on it step by step, the others go to either end (the same target with and without the indefinite stamps).
    st = stamps[-2] if with_indef else indef_case(True, True, m).stamps[-2]
    assert st.n == 129
    target = float(maps_at(st.A, st.mB[:1], st.C, (kC[0] * st.C) ** 0.37 * (kC[1] * st.C) ** 0.63)[1][0])
    return Case(f"indef search {with_indef}", stamps, kC, target, info=info)


# Every committed case: name -> how it is made (made on first use and kept; tests/test_eigen_reference.py holds the reference to the
# 2 % condition on each case with decisions)
SEARCH_CASES = {f"search m={m} q={q}": functools.partial(search_case, m, q) for m in (1, 63, 64, 65) for q in (0.3, 0.7)}
SEARCH_CASES.update({
    "search nbis=0": functools.partial(search_case, 65, 0.3, 0), "search nbis=1": functools.partial(search_case, 65, 0.3, 1),
    "smax": smax_case, "chunk 130": functools.partial(chunk_case, 130, True), "chunk 65": functools.partial(chunk_case, 65, True),
    "resident m=65": functools.partial(resident_case, 65, True), "resident m=200": functools.partial(resident_case, 200, True),
    "indef": functools.partial(indef_case, True), "indef neighbours": functools.partial(indef_case, True, False)})
SINGLE_CASES = {f"size m={m} cond={c:.0e}": functools.partial(size_case, m, c) for m in (1, 63, 64, 65) for c in (1e3, 1e8, 1e11)}
SINGLE_CASES.update({
    "chunk 130": functools.partial(chunk_case, 130, False), "chunk 65": functools.partial(chunk_case, 65, False),
    "resident m=65": functools.partial(resident_case, 65, False), "resident m=200": functools.partial(resident_case, 200, False),
    "indef": functools.partial(indef_case, False)})


# ------------------------------------------------------------------------------------------------ judging a result
def distinct(stamps):
    """[(stamp, [positions])] of the distinct Stamp objects of a batch."""
    seen = {}
    for s, st in enumerate(stamps):
        seen.setdefault(id(st), (st, []))[1].append(s)
    return list(seen.values())


def tied_pixels(case):
    """(pixels whose reference path holds a decision within the bound, pixels, pixels ending strictly inside the bracket)."""
    tied = total = inside = 0
    for st, pos in distinct(case.stamps):
        if st.n == 0:
            continue
        lam, P = st.eig()
        kmin, kmax = case.ends(st)
        k64, margin = bisect(lam, P, st.C, kmin, kmax, case.target, case.smax, case.nbis)
        up = decode(quirk(k64, st.C), st.C, kmin, kmax, case.nbis)[1]
        bound = dec_bound(st.n, cond_sym(lam, kmin), lam[0] + kmin <= 0)
        tied += len(pos) * int((margin < bound).any(1).sum())
        total += len(pos) * case.m
        inside += len(pos) * int((up.any(1) & ~up.all(1)).sum()) if case.nbis else 0
    return tied, total, inside


def quirk(k64, C):
    """The float32 kappa the reference reports for the bisection's kappa (lakernel.py:216-222)."""
    return (k64.astype(np.float32).astype(np.float64) * C).astype(np.float32)


def check_stamp(case, st, T, UC, Sg, kp, tag=""):
    """Statements (a) to (c) for one stamp's outputs T [m][n] float32, UC, Sg, kp [m] float32.  Returns figures for printing:
    dict(tied, s_alone [m] bool, dist_map, dist_dec); raises AssertionError with the figures of the first statement that fails."""
    n, m = st.n, case.m
    lam, P = st.eig()
    kmin, kmax = case.ends(st)
    cond = cond_sym(lam, kmin)
    indef = lam[0] + kmin <= 0
    tc = (C_MAP_INDEF if indef else C_MAP) * cond * EPS
    out = {"tied": 0, "s_alone": np.zeros(m, bool), "dist_dec": 0.0}
    if case.kC.size == 1:
        kap = np.full(m, kmin)
        assert np.allclose(kp, kmin, rtol=1e-6, atol=0), (tag, "kappa")
    else:
        key = ("replay", kmin, kmax, case.target, case.smax, case.nbis, kp.tobytes())
        if key not in st.memo:
            st.memo[key] = replay(lam, P, st.C, kmin, kmax, case.target, case.smax, case.nbis, kp)
        ok, dev, ref, margin, s_alone = st.memo[key]
        assert ok.all(), (tag, "(a) kappa off the grid at pixels", np.flatnonzero(~ok)[:8], kp[~ok][:8])
        wrong = dev != ref
        bound = dec_bound(n, cond, indef)
        out["dist_dec"] = float((margin[wrong] / (max(n, 8) * EPS * cond)).max()) if wrong.any() else 0.0
        bad = wrong & (margin >= bound)
        assert not bad.any(), (tag, "(b) decisions against the reference beyond the bound: (pixel, step)", np.argwhere(bad)[:8],
                               "margins", margin[bad][:8], "bound", bound)
        out["tied"] = int((margin < bound).any(1).sum())
        out["s_alone"] = s_alone.any(1)
        kap = path(~dev, kmin, kmax)[:, -1].astype(np.float64)  # the device's own kappa: the node, free of the float32 store
    key = ("maps", kap.tobytes())
    if key not in st.memo:
        st.memo[key] = maps_at(st.A, st.mB, st.C, kap)
    Tr, Ur, Sr, scale = st.memo[key]
    Tr = Tr.astype(np.float64)
    eT = np.abs(T.astype(np.float64) - Tr).max() / np.abs(Tr).max()
    eU = np.abs(UC - Ur) / np.maximum(np.abs(Ur), scale)
    eS = np.abs(Sg - Sr) / np.abs(Sr)
    out["dist_map"] = float(max(eT - 2 * F32, (eU - RTOL_MAP).max(), (eS - RTOL_MAP).max(), 0.0) / (cond * EPS))
    assert eT <= 2 * F32 + tc, (tag, "(c) T", eT, "cond", cond)
    assert np.all(np.abs(UC - Ur) <= ATOL_MAP + (RTOL_MAP + tc) * np.maximum(np.abs(Ur), scale)), (tag, "(c) UC", eU.max(), "cond", cond)
    assert np.allclose(Sg, Sr, rtol=RTOL_MAP + tc, atol=ATOL_MAP), (tag, "(c) Sigma", eS.max(), "cond", cond)
    return out


# ------------------------------------------------------------------------------------------------ the oracle's own distance
def oracle_distance(case):
    """Distance of the float64 oracle (numpy eigh + the C lakernel1, before any float32 store) from maps_at on one case:
    (over T, UC, Sigma in units of cond eps; over udc and S at mid-bracket and the final kappa in units of max(n, 8) eps cond)."""
    from oracle import oracle as orc

    dist = np.zeros((2, 2))  # [positive definite | indefinite][maps | decisions]
    for st, _ in distinct(case.stamps):
        if st.n == 0:
            continue
        n, m = st.n, case.m
        lam, Q = np.linalg.eigh(st.A)
        P = np.ascontiguousarray(st.mB @ Q)
        kmin, kmax = case.ends(st)
        cond = cond_sym(lam, kmin)
        runs = [(case.nbis if case.kC.size > 1 else 0)] + ([0] if case.kC.size > 1 else [])
        for nb in runs:  # (0 steps: the maps at sqrt(kmin kmax), which is kmin itself for one node)
            k64, S64, U64, tt = np.zeros(m), np.zeros(m), np.zeros(m), np.zeros((m, n))
            orc.lakernel1(lam, Q, P, st.C, case.target, kmin, kmax, nb, k64, S64, U64, tt, case.smax)
            To = tt @ Q.T
            Tr, Ur, Sr, scale = maps_at(st.A, st.mB, st.C, k64)
            eU, eS = (np.abs(U64 - Ur) / np.maximum(np.abs(Ur), scale)).max(), (np.abs(S64 - Sr) / Sr).max()
            eT = np.abs(To - Tr.astype(np.float64)).max() / np.abs(Tr).max()
            cls = int(lam[0] + kmin <= 0)
            dist[cls, 0] = max(dist[cls, 0], max(eT, eU, eS) / (cond * EPS))
            if case.kC.size > 1:
                dist[cls, 1] = max(dist[cls, 1], max((np.abs(U64 - Ur) / scale).max(), eS) / (max(n, 8) * EPS * cond))
    return dist


if __name__ == "__main__":
    worst = np.zeros((2, 2))
    for c in [f() for f in SINGLE_CASES.values()] + [f() for f in SEARCH_CASES.values()]:
        d = oracle_distance(c)
        worst = np.maximum(worst, d)
        line = f"{c.name:32s} oracle: maps {d[0, 0]:7.3f} / {d[1, 0]:7.3f} cond eps, decisions {d[0, 1]:7.3f} / {d[1, 1]:7.3f} max(n,8) eps cond"
        if c.kC.size > 1:
            line += "   tied %d of %d, %d strictly inside" % tied_pixels(c)
        print(line, flush=True)
    print("ORACLE_MAP = %.3g, ORACLE_DEC = %.3g; indefinite stamps: %.3g, %.3g" % (worst[0, 0], worst[0, 1], worst[1, 0], worst[1, 1]))
