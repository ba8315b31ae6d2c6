"""Reference, cases and bounds for the coaddition epilogue (OutStamp._perform_coaddition, coadd.py:1320-1354) on the device layouts:
imcom_coadd_epilogue (coadd_epilogue_kernel<4> / <1> and tsum_stamp_kernel, csrc/la_kernels.hip) and the coaddition inside
imcom_solve_chol_resident_coadd (tile_coadd_partials, csrc/gemm_f64.hip; coadd_from_partials_kernel).  No GPU import: the CPU pin is
tests/test_epilogue_reference.py, the GPU suite tests/test_gpu_epilogue_edges.py.

The reference.  The taper of T is the reference implementation's statement as oracle.trapezoid writes it: the float32 array times
float64 factors in place, row pass then column pass (four roundings to float32 where all four ramps meet).  Everything after it is
summed in long double (64-bit significand here) from the tapered float32 values: v_e = sum of the rows of exposure e, Tsum_inpix =
sum_e v_e, Tsum_stamp_e = sum_a v_e / n2^2, Neff = 1 / sum_e (v_e / sum_e |v_e|)^2 times its own taper, outimage_f = sum_i t_i x_fi.
Neff follows numpy: weight sums that are all zero give 0/0 = NaN (and so does a stamp without pixels, whose other outputs are 0).
The long-double sums' own error is n 2^-64 of the sums of magnitudes, 2^-12 of the bounds below.

Two input families.  EXACT (fade == 0): T = k 2^-12 with integer |k| < 2^11 and indata = k' 2^-8 with |k'| < 2^10.  Every term and
every product is then an integer multiple of 2^-20 below 2^1, and for n <= 4096 every partial sum, in any order, is an integer
multiple of 2^-20 below 2^13: exact in float64.  Tsum_inpix, the per-exposure sums and outimage (ONE rounding of the exact sum to
float32) are determined bit for bit; Tsum_stamp up to its one division; Neff up to the roundings of its own formula.  An indexing
error is a bit mismatch.  REAL (fade > 0, and -B/2 of the fused cases): T = |g| + 0.25 g' with standard normals, float32 -- mostly
positive, so that the weight sums do not cancel: S / sabs <= 4 at every pixel (S = sum_i |t_i|, sabs = sum_e |v_e|) is a condition
on the inputs that the pin test asserts; the bounds use each pixel's own S / sabs.

Bounds, u = 2^-53.  A float32 value and a product of two are exact in float64, so the only errors are those of the additions.  A sum
of n such terms by n - 1 float64 additions IN ANY ORDER (additions of an exact zero are exact, so row groups, register runs, LDS
slots and block-row pieces only change the order) has |error| <= gamma_(n-1) sum |term| <= n u sum |term| (1 + O(n u)) (Higham,
Accuracy and Stability, 4.2); the factor 2 below pays for the second order.
  tapered T     ==                                  every rounding is the reference's own
  Tsum_inpix    2 n u S                              the n rows of the pixel
  Tsum_stamp_e  2 (n + m) u sum_a S_a / n2^2         n u S_a per pixel (S_a >= the exposure's own share), m - 1 additions of the pixels'
                                                     values (<= m u sum_a S_a), one division
  outimage      ulp32(ref) / 2 + 2 n u sum_i |t_i x_i|   the float64 sum as above, then one rounding to float32 (ulp32: the float32
                                                     spacing in the binade of |ref|)
  Neff, rel.    4 n_expo n u (S / sabs) + (3 n_expo + 8) u
                with dv_e the error of v_e (sum_e |dv_e| <= n u S): sabs has relative error n u S / sabs + n_expo u; w_e = v_e / sabs
                has |dw_e| <= |dv_e| / sabs + |w_e| (n u S / sabs + (n_expo + 1) u); q = sum_e w_e^2 has
                |dq| <= 2 sum_e |w_e| |dw_e| + (n_expo + 1) u q <= 2 n u S / sabs (|w_e| <= 1) + q (2 n u S / sabs + (3 n_expo + 3) u),
                and q >= 1 / n_expo (sum_e |w_e| = 1): relative (2 n_expo + 2) n u S / sabs + (3 n_expo + 3) u, the first
                <= 4 n_expo n u S / sabs; the reciprocal adds u, four more u stand for the second order.
                In the exact family dv_e = 0 and the first term is 0; with fade > 0 the four factors of Neff's own taper add 4 u.
In the exact family Tsum_inpix and outimage (against float32(ref)) are held with ==, Tsum_stamp to u |ref| (the one division)."""

from dataclasses import dataclass

import numpy as np

from oracle import oracle as orc

LD = np.longdouble
U = 2.0**-53
CAP = 4.0  # S / sabs of the real family, a condition on the inputs
QUANTITIES = ("T", "Tsum_inpix", "Tsum_stamp", "outimage", "Neff")


# ------------------------------------------------------------------------------------------------ the reference
def reference(Tt, indata, expo, n, n_expo, n2f, n2, fade):
    """Tt [batch][ldn][ldm] f32, indata [batch][n_inframe][ldn] f32, expo [batch][ldn] i32 (the device layouts; rows >= n[s] and columns
    >= m are not read).  Returns a dict: T (list of the tapered float32 [n[s]][m]); outimage [batch][n_inframe][m], Tsum_stamp
    [batch][n_expo], Tsum_inpix and Neff [batch][m] in long double; and what the bounds need: S = sum_i |t_i| and sabs = sum_e |v_e|
    [batch][m], P = sum_i |t_i x_i| [batch][n_inframe][m]; v [batch][m][n_expo], the per-exposure sums."""
    batch, m, nf = len(n), n2f * n2f, indata.shape[1]
    out = dict(T=[], outimage=np.zeros((batch, nf, m), LD), Tsum_stamp=np.zeros((batch, n_expo), LD), Tsum_inpix=np.zeros((batch, m), LD),
               Neff=np.zeros((batch, m), LD), S=np.zeros((batch, m), LD), sabs=np.zeros((batch, m), LD), P=np.zeros((batch, nf, m), LD),
               v=np.zeros((batch, m, n_expo), LD))
    for s in range(batch):
        ns = int(n[s])
        T = np.array(Tt[s, :ns, :m], dtype=np.float32, order="C")
        orc.trapezoid(T.reshape(ns, n2f, n2f), fade)  # (a view: in place)
        out["T"].append(T)
        Tl, e = T.astype(LD), np.asarray(expo[s, :ns])
        assert ns == 0 or (e.min() >= 0 and e.max() < n_expo)
        v = np.stack([Tl[e == q].sum(axis=0) for q in range(n_expo)], axis=1)  # [m][n_expo]
        sabs = np.abs(v).sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            w = v / sabs[:, None]
            neff = 1.0 / np.square(w).sum(axis=1)
        orc.trapezoid(neff.reshape(n2f, n2f), fade)
        x = indata[s, :, :ns].astype(LD)
        out["v"][s], out["sabs"][s], out["S"][s] = v, sabs, np.abs(Tl).sum(axis=0)
        out["Tsum_inpix"][s], out["Tsum_stamp"][s], out["Neff"][s] = v.sum(axis=1), v.sum(axis=0) / LD(n2) ** 2, neff
        out["outimage"][s], out["P"][s] = x @ Tl, np.abs(x) @ np.abs(Tl)
    return out


# ------------------------------------------------------------------------------------------------ the comparator
def ulp32(x):
    """The spacing of float32 in the binade of |x| (x any real; below the normal range: the subnormal spacing)."""
    x = np.abs(np.asarray(x, LD))
    _, e = np.frexp(x)
    return np.ldexp(LD(1.0), np.where(x == 0, -149, np.maximum(e - 24, -149)))


def _ratio(err, bound):
    """max err / bound; a zero bound admits a zero error only."""
    err, bound = np.asarray(err, LD), np.broadcast_to(np.asarray(bound, LD), np.shape(err))
    if err.size == 0:
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, np.where(bound > 0, err / bound, np.inf))
    return float(np.nan_to_num(r, nan=np.inf).max())


def compare(got, ref, case):
    """The worst ratio of error to bound per quantity (a dict over QUANTITIES; > 1: outside the bound, inf: a mismatch where == is
    asked or a NaN out of place).  got: T (per stamp, at least [n[s]][m]: the rows < n[s] and columns < m are looked at; None skips it),
    outimage [batch][n_inframe][m] float32, Tsum_stamp, Tsum_inpix, Neff float64 -- numpy arrays.  case: ns, m, n_expo, n2, fade,
    exact."""
    worst = dict.fromkeys(QUANTITIES, 0.0)
    m, ne = case.m, case.n_expo
    for s, ns in enumerate(case.ns):
        if got["T"] is not None:
            same = np.array_equal(np.asarray(got["T"][s])[:ns, :m], ref["T"][s], equal_nan=True)
            worst["T"] = max(worst["T"], 0.0 if same else np.inf)
        S, sabs = ref["S"][s], ref["sabs"][s]
        r_in, r_st, r_img, r_ne = ref["Tsum_inpix"][s], ref["Tsum_stamp"][s], ref["outimage"][s], ref["Neff"][s]
        g_in, g_st, g_img, g_ne = (np.asarray(got[k][s]) for k in ("Tsum_inpix", "Tsum_stamp", "outimage", "Neff"))
        assert g_img.dtype == np.float32 and g_in.dtype == g_st.dtype == g_ne.dtype == np.float64
        if case.exact:
            b_in, b_st = 0.0, U * np.abs(r_st)
            e_img, b_img = np.abs(g_img.astype(LD) - r_img.astype(np.float32).astype(LD)), 0.0
            first = 0.0
        else:
            b_in, b_st = 2 * ns * U * S, 2 * (ns + m) * U * S.sum() / LD(case.n2) ** 2
            e_img, b_img = np.abs(g_img.astype(LD) - r_img), ulp32(r_img) / 2 + 2 * ns * U * ref["P"][s]
            with np.errstate(invalid="ignore", divide="ignore"):
                first = 4 * ne * ns * U * (S / sabs)
        worst["Tsum_inpix"] = max(worst["Tsum_inpix"], _ratio(np.abs(g_in.astype(LD) - r_in), b_in))
        worst["Tsum_stamp"] = max(worst["Tsum_stamp"], _ratio(np.abs(g_st.astype(LD) - r_st), b_st))
        worst["outimage"] = max(worst["outimage"], _ratio(e_img, b_img))
        nan_r, nan_g = np.isnan(r_ne), np.isnan(g_ne)
        if not np.array_equal(nan_r, nan_g):
            worst["Neff"] = np.inf
        ok = ~nan_r & ~nan_g
        b_ne = (first + (3 * ne + 8 + (4 if case.fade > 0 else 0)) * U) * np.abs(r_ne)
        worst["Neff"] = max(worst["Neff"], _ratio(np.abs(g_ne.astype(LD) - r_ne)[ok], np.broadcast_to(b_ne, r_ne.shape)[ok]))
    return worst


def fmt(worst):
    return ", ".join(f"{k} {worst[k]:.3g}" for k in QUANTITIES)


# ------------------------------------------------------------------------------------------------ inputs
def exposures(pattern, n, n_expo):
    """The exposure of each of n rows.  runs: sorted runs of equal length, as production has them (pixels InStamp by InStamp,
    exposure-major inside); missing: the same with one exposure left out; alternate: another exposure on every row AND on every
    fourth row (what one row group of the kernel sees); back: a return to earlier exposures; single: all rows in one exposure."""
    i = np.arange(n)
    if pattern == "runs":
        e = i * n_expo // max(n, 1)
    elif pattern == "missing":
        e = np.array([0, 1, 3])[i * 3 // max(n, 1)]
    elif pattern == "alternate":
        e = (i + i // 4) % n_expo
    elif pattern == "back":
        e = np.array([0, 1, 0, 2, 3, 1])[i * 6 // max(n, 1)]
    elif pattern == "single":
        e = np.full(n, 2)
    else:
        raise ValueError(pattern)
    assert n == 0 or e.max() < n_expo
    return e.astype(np.int32)


def draw_T(rng, shape, exact):
    if exact:
        return (rng.integers(-(2**11) + 1, 2**11, shape) * 2.0**-12).astype(np.float32)
    return (np.abs(rng.standard_normal(shape)) + 0.25 * rng.standard_normal(shape)).astype(np.float32)


def draw_x(rng, shape, exact):
    if exact:
        return (rng.integers(-(2**10) + 1, 2**10, shape) * 2.0**-8).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float32)


@dataclass(frozen=True)
class Case:
    name: str
    ns: tuple
    n2f: int
    n_expo: int
    n_inframe: int
    n2: int = 0  # 0: n2f (no fade)
    fade: int = 0
    ldn: int = 256
    ldm: int = 0  # 0: the smallest multiple of 128 that holds m
    pattern: str = "runs"
    zero_col: int = -1  # this output column of T is zero on every row
    seed: int = 0

    def __post_init__(self):
        if self.n2 == 0:
            object.__setattr__(self, "n2", self.n2f)
        if self.ldm == 0:
            object.__setattr__(self, "ldm", (self.m + 127) // 128 * 128)
        assert self.n2f == self.n2 + 2 * self.fade and self.ldm % 128 == 0 and self.ldm >= self.m and self.ldn >= max(self.ns)

    @property
    def m(self):
        return self.n2f * self.n2f

    @property
    def exact(self):
        return self.fade == 0

    def inputs(self):
        """Tt [batch][ldn][ldm], indata [batch][n_inframe][ldn], expo [batch][ldn], zero outside the stamps' rows and columns."""
        import zlib

        rng = np.random.default_rng([zlib.crc32(self.name.encode()), self.seed])
        batch = len(self.ns)
        Tt = np.zeros((batch, self.ldn, self.ldm), np.float32)
        x = np.zeros((batch, self.n_inframe, self.ldn), np.float32)
        e = np.zeros((batch, self.ldn), np.int32)
        for s, ns in enumerate(self.ns):
            Tt[s, :ns, : self.m] = draw_T(rng, (ns, self.m), self.exact)
            x[s, :, :ns] = draw_x(rng, (self.n_inframe, ns), self.exact)
            e[s, :ns] = exposures(self.pattern, ns, self.n_expo)
        if self.zero_col >= 0:
            Tt[:, :, self.zero_col] = 0.0
        return Tt, x, e

    def reference(self, data=None):
        Tt, x, e = self.inputs() if data is None else data
        return reference(Tt, x, e, self.ns, self.n_expo, self.n2f, self.n2, self.fade)


ROWS = (0, 1, 3, 4, 5, 15, 16, 17, 31, 33, 64, 200)
FADES = ((1, 1), (2, 3), (10, 3), (8, 1))  # (n2, fade); the first two: ramps that overlap (n2 < 2 fade)


def _cases():
    out = [Case("rows", ROWS, 8, 3, 2), Case("rows-ldn200", ROWS, 8, 3, 2, ldn=200)]
    for n2f in (1, 2, 3, 8, 16, 17):  # m = 1, 4, 9, 64 (one workgroup of the 1-column kernel), 256 (one of the 4-column), 289
        for ne in (3, 9):  # 4 columns a thread, 1 column a thread
            out.append(Case(f"cols-{n2f}-e{ne}", (33, 5, 0, 18), n2f, ne, 2, ldm=128 if n2f * n2f <= 128 else 384))
    for ne, nf in ((1, 1), (1, 4), (2, 5), (6, 2), (8, 8), (9, 3), (9, 9), (64, 1)):
        out.append(Case(f"expo-{ne}-{nf}", (33, 5, 200), 3, ne, nf))
    for pat in ("runs", "missing", "alternate", "back", "single"):
        out.append(Case(f"pattern-{pat}", (33,), 3, 4, 2, pattern=pat))
    out.append(Case("pattern-zerocol", (33,), 3, 4, 2, zero_col=4))
    for n2, fade in FADES:
        for nf in (1, 9):  # one frame pass; three, the later ones on the T the first has tapered
            out.append(Case(f"fade-{n2}-{fade}-f{nf}", (0, 1, 17, 33, 100), n2 + 2 * fade, 3, nf, n2=n2, fade=fade))
    return out


CASES = _cases()


# ------------------------------------------------------------------------------------------------ the fused path
FUSED_NS = (0, 1, 127, 128, 129, 300)
FUSED_LDN = 384
REPAIR_AT = 2  # the stamp of the repair batch whose first factorisation fails


@dataclass(frozen=True)
class FusedCase:
    """One call of imcom_solve_chol_resident_coadd: nv = 1 unless kappaC has two nodes, fade 0, ldn 384.  kind: plain (A = 2 I + a random
    symmetric part of 2-norm 0.4, -B/2 of the real family), identity (A = 0.5 I, kappa = 0.5, -B/2 of the exact family: T = -B/2
    exactly), repair (stamp REPAIR_AT is diag(2) with one entry -0.7 and kappa = 0.5: A + kappa I is indefinite, the repair of
    lakernel.py:262-279 shifts it by 0.7), repair-control (the same batch with an ordinary stamp in that place)."""
    name: str
    n2f: int
    n_expo: int
    n_inframe: int
    kind: str = "plain"
    ns: tuple = FUSED_NS
    kappaC: tuple = (0.01,)
    ldn: int = FUSED_LDN
    fade: int = 0
    seed: int = 0

    @property
    def m(self):
        return self.n2f * self.n2f

    @property
    def n2(self):
        return self.n2f

    @property
    def ldm(self):
        return (self.m + 127) // 128 * 128

    @property
    def exact(self):
        return self.kind == "identity"

    def inputs(self):
        """A [batch][ldn][ldn] (padding: identity), Bt [batch][ldn][ldm] (zero outside the stamps), C [batch], indata, expo."""
        import zlib

        name = self.name.replace("-control", "").replace("-two-nodes", "")  # the variants of one batch share its draws
        rng = np.random.default_rng([zlib.crc32(name.encode()), self.seed])
        batch, ldn = len(self.ns), self.ldn
        A = np.zeros((batch, ldn, ldn))
        Bt = np.zeros((batch, ldn, self.ldm))
        x = np.zeros((batch, self.n_inframe, ldn), np.float32)
        e = np.zeros((batch, ldn), np.int32)
        Cs = np.ones(batch)
        for s, ns in enumerate(self.ns):
            G = rng.standard_normal((ns, ns))
            R = G + G.T
            bad_at = int(rng.integers(0, max(ns, 1)))
            if self.kind == "identity":
                A[s, :ns, :ns] = 0.5 * np.eye(ns)
            elif self.kind == "repair" and s == REPAIR_AT:
                d = np.full(ns, 2.0)
                d[bad_at] = -0.7
                A[s, :ns, :ns] = np.diag(d)
            else:
                A[s, :ns, :ns] = 2.0 * np.eye(ns) + (R * (0.4 / np.linalg.norm(R, 2)) if ns else R)
            A[s, np.arange(ns, ldn), np.arange(ns, ldn)] = 1.0
            Bt[s, :ns, : self.m] = draw_T(rng, (ns, self.m), self.exact)
            x[s, :, :ns] = draw_x(rng, (self.n_inframe, ns), self.exact)
            e[s, :ns] = exposures("runs", ns, self.n_expo)
        return A, Bt, Cs, x, e

    def host_T(self, data=None):
        """Tt as numpy solves it (one node; the repaired stamp with its shift), for the pin of the cap S / sabs."""
        A, Bt, Cs, _, _ = self.inputs() if data is None else data
        Tt = np.zeros(Bt.shape, np.float32)
        for s, ns in enumerate(self.ns):
            M = A[s, :ns, :ns] + self.kappaC[0] * Cs[s] * np.eye(ns)
            if self.kind == "repair" and s == REPAIR_AT:
                M += (0.7 + 1e-16) * np.eye(ns)
            Tt[s, :ns] = np.linalg.solve(M, Bt[s, :ns]) if ns else 0.0
        return Tt


def _fused_cases():
    out = []
    for n2f in (3, 17):  # m = 9 (ldm 128), 289 (ldm 384)
        for ne, nf in ((1, 1), (2, 5), (3, 2), (9, 3)):
            out.append(FusedCase(f"fused-{n2f}-{ne}-{nf}", n2f, ne, nf))
    out.append(FusedCase("fused-identity", 17, 3, 2, kind="identity", kappaC=(0.5,)))
    rep = (17, 127, 200, 128, 129, 300)  # (every n >= 2: with fewer pixels than kappa nodes the reduced system of routine.py:546-588 is singular)
    out.append(FusedCase("fused-repair", 3, 3, 2, kind="repair", ns=rep, kappaC=(0.5,)))
    return out


FUSED_CASES = _fused_cases()
REPAIR_CONTROL = FusedCase("fused-repair-control", 3, 3, 2, kind="repair-control", ns=FUSED_CASES[-1].ns, kappaC=(0.5,))
REPAIR_TWO_NODES = FusedCase("fused-repair-two-nodes", 3, 3, 2, kind="repair", ns=FUSED_CASES[-1].ns, kappaC=(0.5, 0.625))
