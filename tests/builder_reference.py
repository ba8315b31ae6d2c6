"""A high-precision statement of what imcom_build_A / imcom_build_B compute (include/imcom_hip.h), and the inputs on which
tests/test_gpu_builder_edges.py holds the kernels to it.  Plain numpy: nothing of ``oracle`` or ``pyimcom_amd`` is imported.

The operation.  A sample of the pair's table is taken at ``d = a - b; d /= dscale; d += nc; d += 6`` -- float64, in this order,
as the seam defines it -- in x and in y; ``cell = int32(d)`` (truncation) and ``fh = d - cell - 0.5``.  The cell decision is
part of the definition.  A sample with a cell below 4 or above ng - 6 in either axis is off the table.  On the table the value
is ``sum_i wy_i sum_j wx_j f[yc - 4 + i][xc - 4 + j]`` with the D5512 weights of ``fh`` (reference src/pyimcom/routine.py:29-122,
Horner form; the coefficients are those of oracle/imcom_oracle.c).  Here the weights and both sums are ``np.longdouble``,
and every function returns, beside the value, ``S = sum_i |wy_i| sum_j |wx_j| |f_ij|``: the scale a rounding error of the
100-term sum is proportional to -- and ``W = sum_ij (sy_i |wx_j| + |wy_i| sx_j) |f_ij|``, the scale of what the rounding of the
WEIGHTS does to the sum: a float64 Horner evaluation of a weight is off by a few EPS of ``s = getw_scale(fh)`` (the same Horner
forms on absolute values, of order one for every tap), however small the weight itself is.

Tolerance.  A device value is held to ``|device - ref| <= K * EPS * (S + W + |pen|)`` per element -- not to ``max |A|``, under
which a wrong tap order or weight of one sample disappears.  Everything else (off-table samples, negative pair codes, padding,
symmetry, zero rows and columns) is compared with ``==``.

    Why W.  ``K EPS (S + |pen|)`` alone cannot be met by ANY float64 evaluation: where a weight nearly vanishes (fh = -0.5 exactly, as
    on the diagonal of A and at every cell boundary: nine taps are ~1e-9) its absolute rounding error stays ~EPS, i.e. 1e-7 of the
    weight, and when the one tap of weight ~1 meets a small table value the sum inherits it.  The float64 oracle is up to 1.5e8 of
    those units from this module on the cases below (27 on a diagonal element), and 143 on 50 000 uniformly random positions of a
    random table of side 76 (median 0.3).  In units of EPS (S + W + |pen|) the same three sets give 0.72, 0.56 and 0.62.  On an
    ordinary sample W is 3.7 S (median), so the bound below is 14 EPS S there.
    K_ORACLE  the largest distance, in units of EPS (S + W + |pen|), of the float64 oracle (oracle.stamp_system: the reference's own
              operation order, no FMA contraction) from this module over every generated case; measured and asserted by
              tests/test_builder_reference.py.  Measured: 0.56 for A (7.9e4 on-table samples), 0.72 for Bt (4.8e5 outputs).
              Recorded as 0.75.
    K         4 * K_ORACLE = 3: the device groups the same 100 products differently (strip sums of five 16-byte pieces, FMA
              contraction, reversed order for flipped tables), each grouping being one more float64 evaluation of the same sum.

Positions.  Every position that is meant to sit on a cell boundary is an exact binary fraction (positions in multiples of 1/64,
dscale a power of two, integer nc), so that ``d``, the cell and ``fh`` are exact in any arithmetic.
"""

import functools

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
K_ORACLE = 0.75  # measured 0.72 (tests/test_builder_reference.py::test_reference_vs_oracle_and_K prints it); see above
K = 4.0 * K_ORACLE  # the device's bound

PAIR_SWAP, PAIR_FLIP, PAIR_MASK = 1 << 29, 1 << 30, (1 << 28) - 1

# oracle/imcom_oracle.c D5512_EVEN / D5512_ODD: five (even, odd) degree-4 polynomials in fh^2, highest power first
_EVEN = np.array([
    [+1.651881673372979740e-05, -3.145538007199505447e-04, +1.793518183780194427e-03, -2.904014557029917318e-03, +6.187591260980151433e-04],
    [-1.146756217210629335e-04, +2.883845374976550142e-03, -1.857047531896089884e-02, +3.147734488597204311e-02, -6.753293626461192439e-03],
    [+3.256838096371517067e-04, -9.702063770653997568e-03, +8.678848026470635524e-02, -1.659182651092198924e-01, +3.620560878249733799e-02],
    [-4.541830837949564726e-04, +1.494862093737218955e-02, -1.668775957435094937e-01, +5.879306056792649171e-01, -1.367845996704077915e-01],
    [+2.266560930061513573e-04, -7.815848920941316502e-03, +9.686607348538181506e-02, -4.505856722239036105e-01, +6.067135256905490381e-01],
]).astype(LD)
_ODD = np.array([
    [-3.486978652054735998e-06, +6.753750285320532433e-05, -3.871378836550175566e-04, +6.279918076641771273e-04, -1.338434614116611838e-04],
    [+3.121412120355294799e-05, -8.040343683015897672e-04, +5.209574765466357636e-03, -8.847326408846412429e-03, +1.898674086370833597e-03],
    [-1.243658986204533102e-04, +3.804930695189636097e-03, -3.434861846914529643e-02, +6.581033749134083954e-02, -1.436476114189205733e-02],
    [+2.894406669584551734e-04, -9.794291009695265532e-03, +1.104231510875857830e-01, -3.906954914039130755e-01, +9.092432925988773451e-02],
    [-4.336085507644610966e-04, +1.537862263741893339e-02, -1.925091434770601628e-01, +8.993141455798455697e-01, -1.213035309579723942e+00],
]).astype(LD)


class Geom:
    """imcom_table_geom: tables of side ng = nsamp + 12 (a zero border of 6 samples), centre nc, dscale output pixels per sample."""

    def __init__(self, nsamp, dscale, nc=None):
        self.nsamp, self.dscale = int(nsamp), float(dscale)
        self.nc = float(nsamp // 2) if nc is None else float(nc)
        self.ng = self.nsamp + 12


# ------------------------------------------------------------------------------------------------ the operation
def getw(fh):
    """D5512 weights [..., 10] of float64 ``fh`` in long double (routine.py:29-122: taps k and 9 - k are e + o, e - o)."""
    fh = np.asarray(fh, np.float64).astype(LD)
    fh2 = fh * fh
    w = np.empty(fh.shape + (10,), LD)
    for k in range(5):
        ce, co = _EVEN[k], _ODD[k]
        e = (((ce[0] * fh2 + ce[1]) * fh2 + ce[2]) * fh2 + ce[3]) * fh2 + ce[4]
        o = ((((co[0] * fh2 + co[1]) * fh2 + co[2]) * fh2 + co[3]) * fh2 + co[4]) * fh
        w[..., k] = e + o
        w[..., 9 - k] = e - o
    return w


def getw_scale(fh):
    """The same Horner forms on the absolute values of the coefficients and of fh: the scale of the rounding error of a float64
    evaluation of getw (|fl(p(x)) - p(x)| <= gamma_2n p~(|x|), Higham, Accuracy and Stability of Numerical Algorithms, section 5.1).  It is
    of order one for every tap, however small the weight itself is."""
    fh = np.abs(np.asarray(fh, np.float64)).astype(LD)
    fh2 = fh * fh
    w = np.empty(fh.shape + (10,), LD)
    for k in range(5):
        ce, co = np.abs(_EVEN[k]), np.abs(_ODD[k])
        e = (((ce[0] * fh2 + ce[1]) * fh2 + ce[2]) * fh2 + ce[3]) * fh2 + ce[4]
        o = ((((co[0] * fh2 + co[1]) * fh2 + co[2]) * fh2 + co[3]) * fh2 + co[4]) * fh
        w[..., k] = w[..., 9 - k] = e + o
    return w


def position(a, b, geom):
    """Table coordinate of the separation a - b: float64, in the seam's own order."""
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    d = np.array(d, np.float64, ndmin=1)
    d /= geom.dscale
    d += geom.nc
    d += 6.0
    return d


def cell_of(d):
    return np.asarray(d, np.float64).astype(np.int32)  # truncation toward zero (np.int32(x) of routine.py)


def interp_points(table, dx, dy):
    """Scattered samples of one [ngy][ngx] table: (val, S, W, valid, xi, yi); val = S = W = 0 where the sample is off the
    table."""
    ngy, ngx = table.shape
    dx, dy = np.asarray(dx, np.float64), np.asarray(dy, np.float64)
    xi, yi = cell_of(dx), cell_of(dy)
    valid = (xi >= 4) & (xi < ngx - 5) & (yi >= 4) & (yi < ngy - 5)
    val, S, W = np.zeros(dx.shape, LD), np.zeros(dx.shape, LD), np.zeros(dx.shape, LD)
    idx = np.flatnonzero(valid)
    k10 = np.arange(10)
    for c0 in range(0, idx.size, 8192):
        v = idx[c0 : c0 + 8192]
        wx, wy = getw(dx[v] - xi[v] - 0.5), getw(dy[v] - yi[v] - 0.5)
        rows, cols = yi[v, None] - 4 + k10, xi[v, None] - 4 + k10
        f = table[rows[:, :, None], cols[:, None, :]].astype(LD)  # [sample][i: y tap][j: x tap]
        val[v] = ((f * wx[:, None, :]).sum(-1) * wy).sum(-1)
        f, wx, wy = np.abs(f), np.abs(wx), np.abs(wy)
        S[v] = ((f * wx[:, None, :]).sum(-1) * wy).sum(-1)
        sx, sy = getw_scale(dx[v] - xi[v] - 0.5), getw_scale(dy[v] - yi[v] - 0.5)
        W[v] = ((f * sx[:, None, :]).sum(-1) * wy).sum(-1) + ((f * wx[:, None, :]).sum(-1) * sy).sum(-1)
    return val, S, W, valid, xi, yi


def interp_grid(table, dx, dy):
    """The separable grid of routine.py:256-338 for one input pixel: columns at dx[nxo], rows at dy[nyo]; an off-table column or row
    has zero weights (at cell 4).  (val, S, W) as [nyo][nxo], and the raw cells xi[nxo], yi[nyo]."""
    ngy, ngx = table.shape
    dx, dy = np.asarray(dx, np.float64), np.asarray(dy, np.float64)
    xi, yi = cell_of(dx), cell_of(dy)
    vx, vy = (xi >= 4) & (xi < ngx - 5), (yi >= 4) & (yi < ngy - 5)
    xc, yc = np.where(vx, xi, 4), np.where(vy, yi, 4)
    wx = getw(np.where(vx, dx - xi - 0.5, 0.0)) * vx[:, None]
    wy = getw(np.where(vy, dy - yi - 0.5, 0.0)) * vy[:, None]
    k10 = np.arange(10)
    f = table[:, xc[:, None] - 4 + k10].astype(LD)  # [table row][ix][j]
    sx = getw_scale(np.where(vx, dx - xi - 0.5, 0.0)) * vx[:, None]  # (an off-table column or row has exact zeros for weights)
    sy = getw_scale(np.where(vy, dy - yi - 0.5, 0.0)) * vy[:, None]
    strip, astrip, sstrip = (f * wx).sum(-1), (np.abs(f) * np.abs(wx)).sum(-1), (np.abs(f) * sx).sum(-1)  # [table row][ix]
    rows = yc[:, None] - 4 + k10  # [iy][i]
    val = (strip[rows] * wy[:, :, None]).sum(1)
    S = (astrip[rows] * np.abs(wy)[:, :, None]).sum(1)
    W = (sstrip[rows] * np.abs(wy)[:, :, None]).sum(1) + (astrip[rows] * sy[:, :, None]).sum(1)
    return val, S, W, xi, yi


class Ref:
    """Result of ref_A / ref_Bt: ``val`` (long double, penalty included), ``S``, ``W``, ``pen`` and what the coverage assertions need."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def bound(self, k=K):
        return (k * EPS * (self.S + self.W + np.abs(self.pen))).astype(np.float64)


def ref_A(x, y, psf, tables, geom, pair_tab, pair_pen):
    """A[n][n] of ONE stamp: element (i, j), i <= j, from the code of the ordered pair (psf_i, psf_j) -- SWAP: sampled at r_j - r_i,
    FLIP: on np.flip(table), negative: no table -- plus the pair's penalty, mirrored.
    Fields [n][n]: val, S, W, pen, valid (sampled on a table), xi, yi (cells, in the flipped table's frame where flipped; -1 without a
    table), code."""
    x, y, psf = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(psf, np.int64)
    n = x.size
    iu, ju = np.triu_indices(n)
    code = np.asarray(pair_tab, np.int64)[psf[iu], psf[ju]]
    pen = np.asarray(pair_pen, np.float64)[psf[iu], psf[ju]]
    val, S, W = np.zeros(iu.size, LD), np.zeros(iu.size, LD), np.zeros(iu.size, LD)
    valid = np.zeros(iu.size, bool)
    xi, yi = np.full(iu.size, -1, np.int32), np.full(iu.size, -1, np.int32)
    for c in np.unique(code):
        if c < 0:
            continue
        sel = np.flatnonzero(code == c)
        swap, flip, tab = bool(c & PAIR_SWAP), bool(c & PAIR_FLIP), int(c & PAIR_MASK)
        a, b = (ju[sel], iu[sel]) if swap else (iu[sel], ju[sel])
        t = np.flip(tables[tab]) if flip else tables[tab]
        val[sel], S[sel], W[sel], valid[sel], xi[sel], yi[sel] = interp_points(t, position(x[a], x[b], geom), position(y[a], y[b], geom))
    val = val + pen.astype(LD)

    def full(v):
        out = np.zeros((n, n), v.dtype)
        out[iu, ju] = v
        out[ju, iu] = v
        return out

    return Ref(val=full(val), S=full(S), W=full(W), pen=full(pen), valid=full(valid), xi=full(xi), yi=full(yi), code=full(code))


def ref_Bt(x, y, psf, tables, geom, io_tab, out_x0, out_y0, n2f):
    """Bt[n][n2f * n2f] of ONE stamp (output pixel a = iy * n2f + ix at (out_x0 + ix, out_y0 + iy)).
    Fields: val, S, W [n][m], pen (zero), xi, yi [n][n2f] raw cells of the grid's columns / rows, tab [n]."""
    x, y, psf = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(psf, np.int64)
    n, m = x.size, n2f * n2f
    ox, oy = out_x0 + np.arange(n2f, dtype=np.float64), out_y0 + np.arange(n2f, dtype=np.float64)
    val, S, W = np.zeros((n, m), LD), np.zeros((n, m), LD), np.zeros((n, m), LD)
    xi, yi = np.zeros((n, n2f), np.int32), np.zeros((n, n2f), np.int32)
    tab = np.asarray(io_tab, np.int64)[psf]
    for i in range(n):
        v, s, w, xi[i], yi[i] = interp_grid(tables[tab[i]], position(x[i], ox, geom), position(y[i], oy, geom))
        val[i], S[i], W[i] = v.ravel(), s.ravel(), w.ravel()
    return Ref(val=val, S=S, W=W, pen=np.zeros((n, m)), xi=xi, yi=yi, tab=tab)


def grid_rows(yi, ng):
    """Window of table rows a grid's valid rows touch, as grid_pixel takes it: (rlo, rhi, nrows); nrows = 0 without a valid row."""
    ok = (yi >= 4) & (yi < ng - 5)
    if not ok.any():
        return 0, -1, 0
    rlo, rhi = int(yi[ok].min()) - 4, int(yi[ok].max()) + 5
    return rlo, rhi, rhi - rlo + 1


# ------------------------------------------------------------------------------------------------ the cases
def _q64(rng, lo, hi, size):
    """Random multiples of 1/64 in [lo, hi)."""
    return rng.integers(int(round(lo * 64)), int(round(hi * 64)), size) / 64.0


def _gaussian(ns):
    """A smooth, positive table without any symmetry: an off-centre, rotated, anisotropic Gaussian."""
    v, u = np.mgrid[:ns, :ns].astype(np.float64)
    u, v = u - 0.43 * ns, v - 0.56 * ns
    s1, s2 = ns / 5.0, ns / 9.0
    a, b = 0.8 * u + 0.6 * v, -0.6 * u + 0.8 * v
    return np.exp(-0.5 * ((a / s1) ** 2 + (b / s2) ** 2))


def make_tables(rng, ntab, ng, smooth=()):
    """[ntab][ng][ng]: standard-normal samples (no symmetry: flip, swap and transposition all change the value) inside the zero
    border of 6; the tables listed in ``smooth`` are the Gaussian."""
    t = np.zeros((ntab, ng, ng))
    t[:, 6:-6, 6:-6] = rng.standard_normal((ntab, ng - 12, ng - 12))
    for k in smooth:
        t[k, 6:-6, 6:-6] = _gaussian(ng - 12)
    return t


def _pad(rows, ldn, fill, dtype):
    out = np.full((len(rows), ldn), fill, dtype)
    for s, r in enumerate(rows):
        out[s, : len(r)] = r
    return out


def _case_A(name, geom, tables, xs, ys, psfs, ldn, pair_tab, pair_pen, pad_psf):
    """x / y beyond n[s] are NaN; psf beyond n[s] is ``pad_psf``, a valid index."""
    return dict(name=name, geom=geom, tables=tables, n=np.array([len(v) for v in xs], np.int32), ldn=ldn,
                x=_pad(xs, ldn, np.nan, np.float64), y=_pad(ys, ldn, np.nan, np.float64), psf=_pad(psfs, ldn, pad_psf, np.int32),
                pair_tab=np.ascontiguousarray(pair_tab, np.int32), pair_pen=np.ascontiguousarray(pair_pen, np.float64),
                npsf_max=int(pair_tab.shape[-1]))


KINDS = (0, PAIR_FLIP, PAIR_SWAP, PAIR_FLIP | PAIR_SWAP, None)  # None: a negative code


def _codes(P, ntab, shift):
    """[P][P] codes cycling through KINDS over the ordered pairs, tables cycling through the stack, a distinct penalty per pair."""
    tab, pen = np.zeros((P, P), np.int64), np.zeros((P, P))
    for p in range(P):
        for q in range(P):
            e = p * P + q
            kind = KINDS[(e + shift) % 5]
            tab[p, q] = -1 - e if kind is None else (kind | ((e + 2 * shift) % ntab))
            pen[p, q] = (1 + e) / 64.0 * (-1) ** e + shift / 1024.0
    return tab, pen


def _scramble(rng, n, P):
    """PSF indices of n pixels in scrambled order, in which every ordered pair (p, q) occurs as (psf_i, psf_j) with i < j."""
    while True:
        psf = rng.permutation(np.arange(n) % P)
        iu, ju = np.triu_indices(n, 1)
        if np.unique(psf[iu] * P + psf[ju]).size == P * P:
            return psf


RAGGED_N = (0, 1, 15, 16, 17, 127, 128, 129, 200)


def cases_A():
    """Inputs of imcom_build_A (a list of dicts of host arrays, one call each), from fixed seeds.  nsamp = 52 (ng = 64), nc = 26,
    dscale = 0.5: d = 2 (a - b) + 32."""
    out = []
    g = Geom(52, 0.5)
    ng = g.ng
    sep = lambda d: (d - g.nc - 6.0) * g.dscale  # the separation a - b that lands on table coordinate d

    # ragged batch: three PSFs interleaved pixel by pixel, a fourth for the padding; positions over a range whose separations leave
    # the table on both sides now and then
    for ldn in (256, 200):
        rng = np.random.default_rng(7001)
        tables = make_tables(rng, 4, ng, smooth=(1,))
        xs = [_q64(rng, 0.0, 14.25, n) for n in RAGGED_N]
        ys = [_q64(rng, 0.0, 14.25, n) for n in RAGGED_N]
        psfs = [np.arange(n) % 3 for n in RAGGED_N]
        tp = [_codes(4, 4, s) for s in range(len(RAGGED_N))]  # every stamp its own pair table
        out.append(_case_A(f"ragged_ldn{ldn}", g, tables, xs, ys, psfs, ldn, np.stack([t for t, _ in tp]), np.stack([p for _, p in tp]), 3))

    # pair codes: every kind over the ordered pairs, the pair table in LDS (3, 8) and fetched per thread (9); every sample on its table
    for P in (3, 8, 9):
        rng = np.random.default_rng(7100 + P)
        tables = make_tables(rng, 5, ng, smooth=(2,))
        xs = [_q64(rng, 0.0, 12.0, 40) for _ in range(2)]
        ys = [_q64(rng, 0.0, 12.0, 40) for _ in range(2)]
        psfs = [_scramble(rng, 40, P) for _ in range(2)]
        tp = [_codes(P, 5, s) for s in range(2)]
        out.append(_case_A(f"codes_P{P}", g, tables, xs, ys, psfs, 48, np.stack([t for t, _ in tp]), np.stack([p for _, p in tp]), P - 1))

    # boundary cells: anchors at one position; every other pixel is one separation away from them that puts x (y ordinary) or y
    # (x ordinary) at the start / inside / end of cells 3, 4, ng - 6, ng - 5 (d = 3.0 is fh = -0.5 exactly)
    D = [3.0, 3.96875, 4.0, 4.5, ng - 6.0, ng - 6 + 0.96875, ng - 5.0, ng - 5 + 0.5, 32.0]
    ordinary = 30.25
    px, py, pp = [20.0], [21.5], [0]  # anchor 0 (PSF 0) comes first: pairs (anchor, j) are sampled at r_anchor - r_j
    for p in (0, 1):
        for d in D:
            px += [20.0 - sep(d), 20.0 - sep(ordinary)]
            py += [21.5 - sep(ordinary), 21.5 - sep(d)]
            pp += [p, p]
    px, py, pp = px + [20.0, 20.0], py + [21.5, 21.5], pp + [0, 1]  # anchors that come last: SWAP pairs are sampled at r_anchor - r_j
    rng = np.random.default_rng(7200)
    tables = make_tables(rng, 2, ng, smooth=(1,))
    tab = np.array([[0, PAIR_FLIP | 1, 1], [PAIR_SWAP | 1, PAIR_FLIP | PAIR_SWAP | 0, 0], [1, 0, 1]])
    pen = np.array([[0.25, -0.5, 3.0], [0.125, -0.0625, 5.0], [7.0, 9.0, 11.0]])
    out.append(_case_A("boundary", g, tables, [np.array(px)], [np.array(py)], [np.array(pp)], 40, tab[None], pen[None], 2))

    # end of the stack: pairs (0, 1) / (0, 2) on the LAST table, plain / flipped, (0, 3) / (0, 4) the same on the FIRST; the pixels of
    # PSFs 1..4 sit at the separations from the anchor (pixel 0, PSF 0) that hit cells (ng-6, ng-6) and (4, 4); PSF 5 pads
    corner = [ng - 6.0, ng - 6 + 0.75, 4.0, 4.96875]
    for ntab in (1, 3):
        rng = np.random.default_rng(7300 + ntab)
        tables = make_tables(rng, ntab, ng, smooth=(1,) if ntab > 1 else ())
        P = 6
        tab = np.array([[((p + q) % ntab) | (PAIR_FLIP if (p * q) % 2 else 0) for q in range(P)] for p in range(P)])
        tab[0, 1:5] = [ntab - 1, PAIR_FLIP | (ntab - 1), 0, PAIR_FLIP | 0]
        pen = (np.arange(P * P).reshape(P, P) - 7.0) / 32.0
        px, py, pp = [6.0], [7.0], [0]
        for group in ((1, 2), (3, 4)):  # pixels 1..8: the last table, in tile (0, 0); pixels 16..23: the first, in tile (0, 1)
            for p in group:
                for d in corner:
                    px.append(6.0 - sep(d)), py.append(7.0 - sep(d)), pp.append(p)
            fill = 16 - len(px) % 16  # ordinary pixels up to the end of the tile row
            px += list(_q64(rng, 2.0, 10.0, fill)); py += list(_q64(rng, 2.0, 10.0, fill)); pp += list(np.arange(fill) % 3)
        out.append(_case_A(f"stack_end_ntab{ntab}", g, tables, [np.array(px)], [np.array(py)], [np.array(pp)], 48, tab[None], pen[None], 5))
    return out


def stamp_A(case, s):
    """What ref_A takes for stamp s of a case."""
    n = int(case["n"][s])
    return case["x"][s, :n], case["y"][s, :n], case["psf"][s, :n], case["tables"], case["geom"], case["pair_tab"][s], case["pair_pen"][s]


def alone(case, s):
    """Stamp s of a case as a batch of its own (same ldn, same padding)."""
    out = dict(case)
    for k in ("n", "x", "y", "psf", "pair_tab", "pair_pen", "io_tab", "out_x0", "out_y0"):
        if k in case:
            out[k] = np.ascontiguousarray(case[k][s : s + 1])
    out["name"] = f"{case['name']}[{s}]"
    return out


def _case_B(name, geom, tables, d0x, d0y, psfs, ldn, io_tab, out_x0, out_y0, n2f):
    """Pixels are given by the table coordinates (d0x, d0y) of output pixel (0, 0) -- the largest of the grid: column ix sits at
    d0x - ix / dscale -- in multiples of dscale / 64, so that the positions are multiples of 1/64."""
    xs = [x0 + (np.asarray(d, np.float64) - geom.nc - 6.0) * geom.dscale for d, x0 in zip(d0x, out_x0)]
    ys = [y0 + (np.asarray(d, np.float64) - geom.nc - 6.0) * geom.dscale for d, y0 in zip(d0y, out_y0)]
    for v in xs + ys:
        assert np.array_equal(v * 64, np.round(v * 64))
    io_tab = np.ascontiguousarray(io_tab, np.int32)
    return dict(name=name, geom=geom, tables=tables, n=np.array([len(v) for v in xs], np.int32), ldn=ldn,
                x=_pad(xs, ldn, np.nan, np.float64), y=_pad(ys, ldn, np.nan, np.float64), psf=_pad(psfs, ldn, io_tab.shape[1] - 1, np.int32),
                io_tab=io_tab, npsf_max=int(io_tab.shape[1]), out_x0=np.array(out_x0, np.float64), out_y0=np.array(out_y0, np.float64), n2f=n2f)


def _geom_B(n2f):
    """dscale = 0.5: a grid spans 2 (n2f - 1) cells; the table leaves it 16 cells of room."""
    return Geom(2 * (n2f - 1) + 13, 0.5)


def _q32(rng, lo, hi, size):
    return rng.integers(int(round(lo * 32)), int(round(hi * 32)), size) / 32.0


def cases_B():
    """Inputs of imcom_build_B, from fixed seeds."""
    out = []
    # small shapes: three stamps (20, 0 and 7 pixels), two input-output tables (one the last of the stack) and one for the padding
    # PSF; the first pixels reach the last valid cell, the first valid cell, and lose one row / one column
    for n2f in (1, 2, 7, 48):
        g = _geom_B(n2f)
        ng, span = g.ng, 2.0 * (n2f - 1)
        rng = np.random.default_rng(7400 + n2f)
        tables = make_tables(rng, 3, ng, smooth=(1,))
        lo, hi = 4.0 + span, ng - 5.0  # d0 of a grid that lies on the table
        d0x, d0y, psfs = [], [], []
        for n in (20, 0, 7):
            dx, dy = _q32(rng, lo, hi, n), _q32(rng, lo, hi, n)
            if n >= 5:
                dx[:5] = [hi - 0.03125, lo, lo + 3.25, lo - 0.03125, hi]  # last valid cell; first valid cell; inside; last column in cell 3; first in ng - 5
                dy[:5] = [hi - 0.03125, lo, hi, lo + 1.5, lo - 0.03125]  # ...; ...; first row in cell ng - 5; inside; last row in cell 3
            d0x.append(dx), d0y.append(dy), psfs.append(np.arange(n) % 2)
        out.append(_case_B(f"small_n2f{n2f}", g, tables, d0x, d0y, psfs, 22, [[0, 2, 1], [1, 2, 0], [2, 0, 1]], [3.0, 0.0, -2.5], [5.0, 0.0, 7.25], n2f))

    # cut grids: left / right (columns below cell 4 / above ng - 6), top / bottom (rows likewise), a corner, entirely off in y and
    # in x; at n2f = 48 also 7 and 14 rows lost (nrows = 90, 76)
    for n2f in (7, 48):
        g = _geom_B(n2f)
        ng, span = g.ng, 2.0 * (n2f - 1)
        rng = np.random.default_rng(7500 + n2f)
        tables = make_tables(rng, 2, ng, smooth=(0,))
        lo, hi, mid = 4.0 + span, ng - 5.0, 4.0 + span + 7.71875
        d0x = [lo - 5.5, hi + 3.25, mid, hi + 0.25, lo - 3.0, mid, hi + span + 20.0, mid, mid, lo - 200.0]
        d0y = [mid, mid, lo - 4.5, hi + 4.25, hi + 2.0, hi + span + 20.0, mid, lo - 14.0 + 0.46875, hi + 28.0 - 0.5, mid]
        out.append(_case_B(f"cut_n2f{n2f}", g, tables, [d0x], [d0y], [np.arange(10) % 2], 12, [[1, 0, 1]], [-4.0], [9.5], n2f))

    # row-loop tails: n2f = 48 -> nlane = 5, the x-pass walks 15 rows per trip.  dscale = 8: the grid spans 47/8 cells, i.e. 5 or 6
    # depending on the fraction of d0y (nrows = 15, 16); a grid that keeps five valid cells has nrows = 14
    g = Geom(52, 8.0)
    rng = np.random.default_rng(7600)
    tables = make_tables(rng, 2, g.ng, smooth=(1,))
    d0y = [40.875, 40.5, 8.5, 41.0 - 1 / 512, 41.0, 30.873046875, 57.9375, 12.0]
    d0x = [33.25, 40.998046875, 20.5, 11.0, 58.5, 9.875, 30.0, 57.0]
    out.append(_case_B("tails_n2f48", g, tables, [d0x], [d0y], [np.arange(8) % 2], 8, [[0, 1, 0]], [1.0], [-3.0], 48))

    # fallback: n2f = 48 on a table of side 449.  dscale = 0.125: 47 * 8 + 10 = 386 rows do not fit the 96 KB window -> the direct
    # 100-tap form; the SAME pixels at dscale = 0.5 go through the LDS form.  One pixel loses rows and columns.
    rng = np.random.default_rng(7700)
    tables = make_tables(rng, 2, 449, smooth=(0,))
    offx = np.array([19.5, 27.421875, 23.015625, 25.5, 17.0, 21.25])  # x_in - out_x0; on the table at dscale 0.125: [19.5, 27.5)
    offy = np.array([27.0, 19.5, 24.984375, 20.125, 28.5, 26.0])
    for name, ds in (("fallback_direct", 0.125), ("fallback_lds", 0.5)):
        g = Geom(437, ds)
        out.append(_case_B(name, g, tables, [offx / ds + g.nc + 6.0], [offy / ds + g.nc + 6.0], [np.arange(6) % 2], 6, [[0, 1, 0]], [2.0], [-1.0], 48))

    # wide grid: n2f = 257 > 256 threads.  The 96 KB budget holds 26 rows: dscale = 32 (256/32 + 10 = 18 rows) takes the LDS form,
    # dscale = 8 (42 rows) the direct one.  Two pixels of each leave the table.
    rng = np.random.default_rng(7800)
    tables = make_tables(rng, 2, 64, smooth=(1,))
    for name, ds, d0x, d0y in (("wide_lds", 32.0, [41.3828125, 12.0, 60.0], [58.998046875, 10.5, 33.0]),
                               ("wide_direct", 8.0, [40.125, 58.873046875, 30.0], [36.0, 50.5, 61.5])):
        out.append(_case_B(name, Geom(52, ds), tables, [d0x], [d0y], [np.arange(3) % 2], 3, [[1, 0, 1]], [-7.0], [4.0], 257))
    return out


def stamp_B(case, s):
    """What ref_Bt takes for stamp s of a case."""
    n = int(case["n"][s])
    return (case["x"][s, :n], case["y"][s, :n], case["psf"][s, :n], case["tables"], case["geom"], case["io_tab"][s],
            float(case["out_x0"][s]), float(case["out_y0"][s]), case["n2f"])


def grid_lds_rows(n2f, dscale):
    """max_rows of launch_build_B (grid_lds in pyimcom_amd/csrc/interp.hip restated): the rows of n2f doubles that the x-pass window
    may hold -- the caller's hint (n2f - 1) / dscale + 13, inside a 96 KB budget; 0 = direct form only."""
    fixed = 10 * (2 * n2f) * 8 + (2 * n2f + 4) * 4
    budget = 96 * 1024
    rows = (budget - fixed) // (n2f * 8) if fixed < budget else 0
    hint = int((n2f - 1) / dscale) + 13
    if 0 < hint < rows:
        rows = hint
    rows = min(rows, 4096)
    return rows if rows >= 10 else 0


@functools.lru_cache(maxsize=None)
def refs_A():
    """[(case, [ref_A of every stamp])], computed once per process and shared by the tests; nobody writes to it."""
    return [(c, [ref_A(*stamp_A(c, s)) for s in range(c["n"].size)]) for c in cases_A()]


@functools.lru_cache(maxsize=None)
def refs_B():
    return [(c, [ref_Bt(*stamp_B(c, s)) for s in range(c["n"].size)]) for c in cases_B()]
