"""High-precision reference and case builder for the conjugate-gradient solvers of the Iterative kernel (csrc/iter_block.hip,
csrc/iter_empir.hip iter_cg_kernel).  No GPU and no library import: numpy and the Python oracle only.

The reference is lakernel.conjugate_gradient (lakernel.py:397-442) and IterKernel._iterative_wrapper (545-586) restated in
np.longdouble.  The cases are WELL-conditioned on purpose (kappa/C of a few tenths, cond < 100): there CG is not sensitive to rounding
-- float64 CG in natural and in reversed index order stays within 1e-16 .. 2e-12 of the long-double run -- so the device can be held per
element to float32 rounding of the reference and to EQUAL step counts, and a dropped tile, mask bit or ring piece is orders of magnitude
outside the bound (tests/test_iter_reference.py shows that on the host; tests/test_gpu_iter_edges.py applies it on the device).
"""

import functools
from dataclasses import dataclass

import numpy as np

LD = np.longdouble

RHO = 4.0       # acceptance radius in output pixels
C_OUT = 0.7     # out-out overlap C of every case
KAPPA_C = 0.3   # kappa / C: cond(A + kappa) stays below 100 for every committed case (test_iter_reference.py asserts it)
NOISE = 0.3     # weight of the rough part of -B/2 (system)
RTOL_STOP, MAXITER_STOP = 1.5e-3, 64  # the stopping mode: the reference's default tolerance (ITERRTOL)
MAXITER_FIXED = 6                     # the fixed mode: rtol = 0, six steps


def cg_ld(A, b, rtol, maxiter, product=None):
    """lakernel.conjugate_gradient (lakernel.py:397-442) in np.longdouble, statement for statement like oracle.conjugate_gradient.
    Returns x, the steps taken and the ratios |r| / atol tested at the top of every step (inf where atol = 0).  ``product`` (test
    instrumentation: tests/test_iter_reference.py damages the matrix product with it) replaces q = A @ p."""
    A, b = np.asarray(A, dtype=LD), np.asarray(b, dtype=LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        atol = np.sqrt(np.dot(b, b)) * LD(rtol)
        x = np.zeros_like(b)
        r = b.copy()
        rho_prev = LD(0.0)
        p = r.copy()
        steps, ratios = 0, []
        for iteration in range(maxiter):
            rho_cur = np.dot(r, r)
            ratios.append(float(np.sqrt(rho_cur) / atol) if atol > 0 else np.inf)
            if np.sqrt(rho_cur) < atol:
                break
            if iteration > 0:
                p *= rho_cur / rho_prev
                p += r
            q = A @ p if product is None else product(A, p)
            alpha = rho_cur / np.dot(p, q)
            x += alpha * p
            r -= alpha * q
            rho_prev = rho_cur
            steps += 1
    return x, steps, ratios


def solve_patchwise(A, diag_add, mBhalf, relevant, rtol, maxiter):
    """IterKernel._iterative_wrapper (lakernel.py:545-586) on AA = A with ``diag_add`` added to the diagonal in float64 (630-632): one
    cg_ld per output pixel on its own selection.  Returns T (float64 [m][n], BEFORE the reference's float32 cast), the steps [m] and the
    tested ratios per pixel."""
    m, n = mBhalf.shape
    AA = np.array(A, dtype=np.float64)
    if diag_add:
        AA[np.diag_indices(n)] += diag_add
    T, steps, ratios = np.zeros((m, n)), np.zeros(m, dtype=np.int64), []
    for a in range(m):
        sel = np.nonzero(relevant[a])[0]
        x, k, rat = cg_ld(AA[np.ix_(sel, sel)], mBhalf[a, sel], rtol, maxiter)
        T[a, sel] = x.astype(np.float64)
        steps[a] = k
        ratios.append(rat)
    return T, steps, ratios


def bound(x_ld, ref_err):
    """Per-element bound on |device T - x_ld|: 2^-24 |x_ld| for the float32 cast of T (|fl(y) - x| <= |fl(y) - y| + |y - x|) plus ten
    times the reference's own float64 distance (``ref_err``, relative to max |x|: the project's convention, README "10 ref_err")."""
    x_ld = np.abs(np.asarray(x_ld, dtype=np.float64))
    return 2.0**-24 * x_ld + 10.0 * ref_err * x_ld.max(axis=-1, keepdims=True)


@dataclass
class Case:
    n: int            # input pixels (union + outside)
    ldn: int          # leading dimension of the padded arrays (> n)
    m: int            # output pixels
    W: int            # width of the output grid
    n_union: int      # union selection of every 4 x 4 patch that is not empty (one patch unless stated)
    A: np.ndarray     # [n][n]
    mBhalf: np.ndarray  # [m][n]
    oy: np.ndarray
    ox: np.ndarray
    iy: np.ndarray
    ix: np.ndarray
    rho: float
    C: float
    kappaC: float
    relevant: np.ndarray  # [m][n] bool, oracle._relevant

    @property
    def kappa(self):
        return self.kappaC * self.C

    def padded(self):
        """The arrays of an imcom_solve_iter call with leading dimension ldn.  What lies beyond n is NOT neutral: matrix entries, -B/2
        and coordinates there would be selected (they sit on the grid's centre) and would move the result if the library looked."""
        n, ldn, m = self.n, self.ldn, self.m
        Ap, Bp = np.full((ldn, ldn), 3.0), np.full((m, ldn), -2.0)
        Ap[:n, :n], Bp[:, :n] = self.A, self.mBhalf
        yp, xp = np.full(ldn, self.oy.mean()), np.full(ldn, self.ox.mean())
        yp[:n], xp[:n] = self.iy, self.ix
        return Ap, Bp, np.stack([self.oy, self.ox]), yp, xp


def patch_unions(relevant, m, W):
    """Union selection (bool [n]) of every 4 x 4 patch of the output grid, patch-row major as csrc/iter_block.hip bcg_pixel."""
    H = (m + W - 1) // W
    out = []
    for by in range((H + 3) // 4):
        for bx in range((W + 3) // 4):
            pix = [y * W + x for y in range(4 * by, min(4 * by + 4, H)) for x in range(4 * bx, min(4 * bx + 4, W)) if y * W + x < m]
            out.append((pix, relevant[pix].any(axis=0)))
    return out


def system(iy, ix, oy, ox, rng, w, wb=2.0, c=0.002):
    """A = 0.7 exp(-d^2 / 2 w^2) + c u u^T (u positive: no 16 x 16 tile of any sub-matrix is negligible) and a dense -B/2 that is
    non-zero outside the discs too."""
    n = iy.size
    u, v = rng.uniform(0.8, 1.2, n), rng.uniform(0.5, 1.5, n)
    A = 0.7 * np.exp(-((ix[:, None] - ix[None]) ** 2 + (iy[:, None] - iy[None]) ** 2) / (2.0 * w * w)) + c * np.outer(u, u)
    B = 0.7 * np.exp(-((ix[None] - ox[:, None]) ** 2 + (iy[None] - oy[:, None]) ** 2) / (2.0 * wb * wb))
    B += 0.05 * v[None] * (1.0 + 0.1 * np.arange(oy.size)[:, None])
    # a rough part whose weight differs from pixel to pixel: the recurrences of one patch then stop at different steps
    B += NOISE * ((np.arange(oy.size) % 5) / 4.0)[:, None] * rng.standard_normal(n)[None]
    return A, B


def make_case(n_union, rng, m_side=(4, 4), n_outside=None, ldn=None, rho=RHO, w0=0.5):
    """A system with geometry whose patch union is EXACTLY ``n_union`` rows: output pixels on an m_side grid of unit spacing, points
    inside every disc, points on the rim (selected by some but not all pixels: 40 % of the union where the grid has more than one pixel),
    ``n_outside`` points outside every disc, all in random index order (the union is not contiguous), ldn > n.  The Gaussian's width
    follows the density (w = w0 x the mean spacing), so the spectrum -- and with it the conditioning -- is alike at every size."""
    from oracle import oracle as orc

    my, mx = m_side
    m = my * mx
    oy, ox = np.repeat(np.arange(my, dtype=np.float64), mx), np.tile(np.arange(mx, dtype=np.float64), my)
    cy, cx, hd = (my - 1) / 2.0, (mx - 1) / 2.0, 0.5 * np.hypot(my - 1, mx - 1)
    n_rim = (2 * n_union + 4) // 5 if m > 1 and n_union >= 4 else 0
    n_in = n_union - n_rim
    if n_outside is None:
        n_outside = max(3, n_union // 8)
    want = {"in": n_in, "rim": n_rim, "out": n_outside}
    got = {k: [] for k in want}
    R = rho + hd + 2.0
    while any(len(got[k]) < want[k] for k in want):
        py, px = rng.uniform(cy - R, cy + R, 4096), rng.uniform(cx - R, cx + R, 4096)
        d = np.hypot(oy[:, None] - py[None], ox[:, None] - px[None])
        clear = (np.abs(d - rho) > 1e-6).all(axis=0)  # no point near a disc's edge: hypot may differ by an ulp between host and device
        cnt = (d < rho).sum(axis=0)
        for k, msk in (("in", cnt == m), ("rim", (cnt > 0) & (cnt < m)), ("out", cnt == 0)):
            for j in np.nonzero(msk & clear)[0][: want[k] - len(got[k])]:
                got[k].append((py[j], px[j]))
    pts = np.array(got["in"] + got["rim"] + got["out"]).reshape(-1, 2)
    while True:  # random index order in which the union's members are not one contiguous run
        perm = rng.permutation(pts.shape[0])
        if m == 1 or n_outside == 0 or n_union < 2 or np.ptp(np.nonzero(perm < n_union)[0]) + 1 > n_union:
            break
    pts = pts[perm]
    iy, ix = np.ascontiguousarray(pts[:, 0]), np.ascontiguousarray(pts[:, 1])
    n = iy.size
    w = w0 * np.sqrt(np.pi * (rho + 0.5 * hd) ** 2 / max(n_union, 1))
    A, B = system(iy, ix, oy, ox, rng, w)
    relevant = orc._relevant(oy, ox, iy, ix, rho)
    case = Case(n=n, ldn=n + 5 if ldn is None else ldn, m=m, W=mx, n_union=n_union, A=A, mBhalf=B, oy=oy, ox=ox, iy=iy, ix=ix, rho=rho,
                C=C_OUT, kappaC=KAPPA_C, relevant=relevant)
    # the builder's own conditions
    assert case.ldn > n
    for pix, un in patch_unions(relevant, m, mx):
        assert un.sum() == n_union, (un.sum(), n_union)
    assert relevant.any(axis=1).all(), "every output pixel selects something"
    some, all_ = relevant.any(axis=0), relevant.all(axis=0)
    if m > 1:
        assert (some & ~all_).sum() >= n_union // 4
        assert n_outside == 0 or n_union < 2 or np.ptp(np.nonzero(some)[0]) + 1 > n_union, "the union is not contiguous"
    assert np.abs(A).min() >= 1e-3 * np.abs(A).max()
    return case


# ---- the committed cases: (family, n_union) -> Case, the same in the CPU and the GPU suite --------------------------------------------
MULTIPLES = (16, 208, 224, 464, 480, 512, 528, 720, 736, 768, 784, 864)  # ring depth, transposition tiles, templates (launch_iter_block)
SWEEP = tuple(sorted(set([16 * t - 5 for t in range(1, 55)]) | set(MULTIPLES) | {1, 15, 17}))  # the half-storage kernel
SWEEP_STOP = tuple(sorted(set(MULTIPLES) | {u + d for u in MULTIPLES for d in (-1, 1) if u + d <= 864}))
FULL_NTILE = (1, 2, 4, 5, 8, 9, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
FULL = tuple(16 * t - 5 for t in FULL_NTILE) + (1024,)  # IMCOM_ITER_SYM=0
FULL_STOP = tuple(16 * t - 5 for t in (9, 17, 32, 33, 48, 49)) + (1024,)  # chunk tails of the prefetch and the three templates
FULL_DEFAULT = (865, 880, 1024)  # full storage without the switch
PER_PIXEL = (1, 255, 256, 257, 511, 513)  # IMCOM_ITER_PER_PIXEL=1, m = 16
PER_PIXEL_ONE = (4095, 4096)  # m = 1


@functools.lru_cache(maxsize=None)
def case_for(n_union, m_side=(4, 4)):
    """The committed case of a union size: seed = the size itself (m = 16) or 7 + the size (m = 1)."""
    if m_side == (4, 4):
        return make_case(n_union, np.random.default_rng(n_union))
    return make_case(n_union, np.random.default_rng(7 + n_union), m_side=m_side, n_outside=16)


@functools.lru_cache(maxsize=None)
def reference(n_union, m_side, rtol, maxiter):
    """(T_ld, steps, ratios, ref_err) of a committed case.  ref_err: the larger of |float64 oracle.conjugate_gradient - cg_ld| / max |x|
    over the pixels, with every selection in natural and in reversed index order."""
    from oracle import oracle as orc

    c = case_for(n_union, m_side)
    T, steps, ratios = solve_patchwise(c.A, c.kappa, c.mBhalf, c.relevant, rtol, maxiter)
    AA = c.A + c.kappa * np.eye(c.n)
    err = 0.0
    for a in range(c.m):
        sel = np.nonzero(c.relevant[a])[0]
        for s in (sel, sel[::-1]):
            x = orc.conjugate_gradient(AA[np.ix_(s, s)], c.mBhalf[a, s].copy(), rtol, maxiter)
            err = max(err, np.abs(x - T[a, s]).max() / np.abs(T[a, s]).max())
    T.setflags(write=False)
    return T, steps, ratios, err


def fixed_maxiter(n_union, m_side=(4, 4)):
    """Steps of the fixed mode: six, but never more than the smallest selection has rows -- CG ends after as many steps as the system has
    rows, and a further step divides a residual of exactly zero by itself (in any arithmetic: the one-row cases)."""
    return min(MAXITER_FIXED, int(case_for(n_union, m_side).relevant.sum(axis=1).min()))


# ---- the ragged batch: three stamps with n = (~900, 0, 3) on a 9 x 6 grid with 50 output pixels ---------------------------------------
RAGGED_W, RAGGED_M, RAGGED_RHO = 9, 50, 2.0


@functools.lru_cache(maxsize=None)
def ragged_batch():
    """Stamps [Case, None, Case] sharing one output grid (W = 9, six rows, the last of five pixels: partial columns, rows and last row)
    and one ldn.  Stamp 0: the six patches hold unions of 728, 100, 0, 10, 40 and 5 rows -- every cluster of input pixels lies where only
    the pixels of ONE patch reach it; the 10-row patch leaves two of its pixel columns with empty discs.  Stamp 1: n = 0.  Stamp 2: three
    input pixels next to each other (a selection holds all of them or none)."""
    from oracle import oracle as orc

    rng = np.random.default_rng(2024)
    W, m, rho = RAGGED_W, RAGGED_M, RAGGED_RHO
    a = np.arange(m)
    oy, ox = (a // W).astype(np.float64), (a % W).astype(np.float64)
    patch_of = (a // W // 4) * ((W + 3) // 4) + (a % W) // 4
    # (target patch or -1 = outside every disc, count, box y0 y1 x0 x1)
    clusters = [(0, 728, -1.4, 1.6, -1.4, 1.6), (1, 100, -1.0, 1.9, 5.05, 5.9), (3, 10, 5.3, 5.7, -0.2, 0.2), (4, 40, 4.2, 5.8, 5.1, 5.95),
                (5, 5, 3.8, 4.2, 9.3, 9.7), (-1, 30, -9.0, -3.0, -3.0, 12.0)]
    pts = []
    for target, count, y0, y1, x0, x1 in clusters:
        got = 0
        while got < count:
            py, px = rng.uniform(y0, y1, 1024), rng.uniform(x0, x1, 1024)
            d = np.hypot(oy[:, None] - py[None], ox[:, None] - px[None])
            rel = d < rho
            ok = (np.abs(d - rho) > 1e-6).all(axis=0)
            for j in range(1024):
                reach = set(patch_of[rel[:, j]])
                if ok[j] and reach == ({target} if target >= 0 else set()) and got < count:
                    pts.append((py[j], px[j]))
                    got += 1
    pts = np.array(pts)[rng.permutation(len(pts))]
    iy, ix = np.ascontiguousarray(pts[:, 0]), np.ascontiguousarray(pts[:, 1])
    A, B = system(iy, ix, oy, ox, rng, 0.05)
    ldn = iy.size + 11
    big = Case(n=iy.size, ldn=ldn, m=m, W=W, n_union=728, A=A, mBhalf=B, oy=oy, ox=ox, iy=iy, ix=ix, rho=rho, C=C_OUT, kappaC=KAPPA_C,
               relevant=orc._relevant(oy, ox, iy, ix, rho))
    ty, tx = 2.5 + rng.uniform(-0.01, 0.01, 3), 4.0 + rng.uniform(-0.01, 0.01, 3)
    A3, B3 = system(ty, tx, oy, ox, rng, 0.01)
    small = Case(n=3, ldn=ldn, m=m, W=W, n_union=3, A=A3, mBhalf=B3, oy=oy, ox=ox, iy=ty, ix=tx, rho=rho, C=0.65, kappaC=KAPPA_C,
                 relevant=orc._relevant(oy, ox, ty, tx, rho))
    # the conditions of the batch, from the host's acceptance masks
    sizes = [int(un.sum()) for _, un in patch_unions(big.relevant, m, W)]
    assert sizes == [728, 100, 0, 10, 40, 5], sizes
    assert max(sizes) >= 600 and 0 < min(s for s in sizes if s) <= 16 and 0 in sizes
    pix3, un3 = patch_unions(big.relevant, m, W)[3]
    assert un3.any() and not big.relevant[pix3].any(axis=1).all(), "a non-empty patch with an empty disc"
    for c in (big, small):
        k = c.relevant.sum(axis=1)
        assert ((k == 0) | (k >= 2)).all(), "no one-row selection (its recurrence ends after one step)"
    assert set(small.relevant.sum(axis=1)) == {0, 3}
    return [big, None, small]


@functools.lru_cache(maxsize=None)
def ragged_reference(rtol, maxiter):
    """Per stamp of ragged_batch(): (T_ld, steps, ref_err) or None."""
    from oracle import oracle as orc

    out = []
    for c in ragged_batch():
        if c is None:
            out.append(None)
            continue
        T, steps, _ = solve_patchwise(c.A, c.kappa, c.mBhalf, c.relevant, rtol, maxiter)
        AA = c.A + c.kappa * np.eye(c.n)
        err = 0.0
        for a in range(c.m):
            sel = np.nonzero(c.relevant[a])[0]
            for s in (sel, sel[::-1]):
                if s.size:
                    x = orc.conjugate_gradient(AA[np.ix_(s, s)], c.mBhalf[a, s].copy(), rtol, maxiter)
                    err = max(err, np.abs(x - T[a, s]).max() / np.abs(T[a, s]).max())
        T.setflags(write=False)
        out.append((T, steps, err))
    return out
