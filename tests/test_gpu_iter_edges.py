"""The conjugate-gradient solvers of the Iterative kernel called directly (imcom_solve_iter, host buffers) at the sizes where their
control flow changes, against the long-double reference of tests/iter_reference.py -- per element, with EQUAL step counts.

What launch_iter_block (csrc/iter_block.hip) does with the largest union of a call, ups = 16 ntile, eight waves, 160 KB of LDS:
  half storage (iter_block_cg_sym_kernel)   ups <= 864;  ring depth 3 for ups <= 208, 2 for 224 .. 464, 1 for 480 .. 864; two transposition
                                            tiles per wave up to ups 720, one from 736; <4, false> for ntile <= 32, <6, false> <= 48,
                                            <7, true> <= 54; the loop over the panels beyond a wave's last row runs from ntile 26 (<4>),
                                            42 (<6>) and 50 (<7>)
  full storage (iter_block_cg_kernel)       ups 880 .. 1024, and every union with IMCOM_ITER_SYM=0: <8> for ntile <= 32, <12> <= 48, <16>
                                            beyond; eight k-tiles fetched ahead (tails at ntile 1 .. 9, 16 / 17)
  per pixel (iter_cg_kernel)                a union above 1024, and IMCOM_ITER_PER_PIXEL=1: 256 threads, 16 rows each, 4096 rows at most
Every case runs in two modes.  FIXED: rtol = 0, six steps; every element of T within iter_reference.bound of the sixth long-double
iterate, T == 0 exactly off the discs and in the padding columns, six steps everywhere.  STOPPING (at the boundary sizes): rtol = 1.5e-3;
the per-pixel step counts EQUAL the reference's and T is within the bound of its result.  The cases are well-conditioned (cond < 100), so
the reference's own float64 distance ref_err is 1e-16 .. 2e-12 and the bound is float32's rounding of T, 2^-24 |x|, plus 10 ref_err max |x|.
A one-row system (union 1) runs ONE fixed step: CG ends after as many steps as the system has rows, a further step divides 0 by 0.

MEASURED on the MI355X (every case prints its figures): T equals float32(x_longdouble) bit for bit in every case -- 0 of 583 k elements
(half storage), 0 of 211 k (full storage), 0 of 80 k (per pixel), 0 of 16 k (ragged batch) differ; the largest |T - x| / bound is 0.998
(half), 0.996 (full), 0.994 (per pixel), all of it the float32 rounding of T; the part of |T - x| beyond 2^-24 |x| is 0 x ref_err
everywhere, so the device's float64 distance / ref_err is below what a float32 T resolves (DESIGN.md "Iterative kernel: edge suite",
also for the two scratch mutants that show where the suite bites).
"""

import ctypes as C

import numpy as np
import pytest

from tests import iter_reference as ir

pytestmark = pytest.mark.gpu

SWITCHES = ("IMCOM_ITER_SYM", "IMCOM_ITER_PER_PIXEL", "IMCOM_ITER_BUDGET_MB")


def _switches(monkeypatch, **kw):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv(k, str(v))


def _solve(stamps, rtol, maxiter, T_fill=np.nan):
    """One imcom_solve_iter call (one kappa node, approximate U/C as the reference's single-node default) on a batch of
    iter_reference.Case (None = a stamp without input pixels).  Returns T, UC, Sigma, kappa, stats, steps."""
    from pyimcom_amd._lib import MEM_HOST, check, default_context, lib

    first = next(c for c in stamps if c is not None)
    batch, m, ldn = len(stamps), first.m, first.ldn
    A, B = np.full((batch, ldn, ldn), 3.0), np.full((batch, m, ldn), -2.0)
    yx, iy, ix = np.zeros((batch, 2, m)), np.zeros((batch, ldn)), np.zeros((batch, ldn))
    Cs, n_arr = np.full(batch, 0.66), np.zeros(batch, dtype=np.int32)
    for s, c in enumerate(stamps):
        yx[s] = np.stack([first.oy, first.ox])
        if c is not None:
            assert c.m == m and c.ldn == ldn
            A[s], B[s], yx[s], iy[s], ix[s] = c.padded()
            Cs[s], n_arr[s] = c.C, c.n
    kC = np.array([first.kappaC])
    T = np.full((batch, m, ldn), T_fill, dtype=np.float32)
    UC, Sg, kp = (np.full((batch, m), np.nan, dtype=np.float32) for _ in range(3))
    ctx = default_context()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    try:
        check(lib.imcom_solve_iter(ctx.handle, batch, p(n_arr), ldn, m, p(A), p(B), p(Cs), p(kC), 1, 1e-6, 0.5, p(yx), p(iy), p(ix),
                                   first.rho, rtol, maxiter, 0, p(T), p(UC), p(Sg), p(kp), MEM_HOST))
    except Exception as e:  # (the caller of the 4097-row case looks at T)
        e.T = T
        raise
    stats, steps = ctx.iter_stats(batch * m)
    return T, UC, Sg, kp, stats, steps.reshape(batch, m)


def _check_stamp(c, T, UC, Sg, kp, steps, T_ld, steps_ld, ref_err, tag, check_steps=None):
    """One stamp of a call against its reference: T per element, the support of T, the steps, and the maps -- the reference's formulas
    (lakernel.py:634-654) in float64 on the device's own T, with the tolerances of test_gpu_iter_empir.py::_check_ill_posed_target."""
    n = c.n
    bd = ir.bound(T_ld, ref_err)
    d = np.abs(T[:, :n].astype(np.float64) - T_ld)
    scale = np.abs(T_ld).max(axis=1, keepdims=True)
    scale[scale == 0] = 1.0
    with np.errstate(invalid="ignore", divide="ignore"):
        used = np.nanmax(np.where(bd > 0, d / bd, 0.0))
    excess = np.maximum(d - 2.0**-24 * np.abs(T_ld), 0.0) / scale
    flips = int((T[:, :n] != T_ld.astype(np.float32)).sum())  # elements on the other side of a float32 rounding boundary than float32(x)
    print(f"[iter-edges] {tag}: |T - x| / bound <= {used:.3f}, excess / ref_err = {excess.max() / max(ref_err, 1e-300):.3g} (ref_err {ref_err:.1e}), "
          f"T != float32(x) at {flips} of {int(c.relevant.sum())} elements")
    assert np.isfinite(T).all()
    assert (d <= bd).all(), (tag, used)
    assert not T[:, :n][~c.relevant].any() and not T[:, n:].any(), "T == 0 off the discs and in the padding columns"
    rows = np.ones(c.m, bool) if check_steps is None else check_steps
    assert np.array_equal(steps[rows], steps_ld[rows]), (tag, steps, steps_ld)
    T64 = T[:, :n].astype(np.float64)
    D, N = np.einsum("ai,ai->a", c.mBhalf, T64), np.einsum("ai,ai->a", T64, T64)
    assert np.array_equal(kp, np.full(c.m, c.kappa).astype(np.float32))
    assert np.allclose(Sg, N, rtol=1e-5, atol=0)
    assert np.allclose(UC, 1.0 - (c.kappa * N + D) / c.C, rtol=1e-5, atol=5e-6)


def _run_case(n_union, mode, m_side=(4, 4), family=""):
    c = ir.case_for(n_union, m_side)
    rtol, maxiter = (0.0, ir.fixed_maxiter(n_union, m_side)) if mode == "fixed" else (ir.RTOL_STOP, ir.MAXITER_STOP)
    T_ld, steps_ld, _, err = ir.reference(n_union, m_side, rtol, maxiter)
    T, UC, Sg, kp, stats, steps = _solve([c], rtol, maxiter)
    if mode == "fixed":
        assert (steps_ld == maxiter).all()
    _check_stamp(c, T[0], UC[0], Sg[0], kp[0], steps[0], T_ld, steps_ld, err, f"{family} union {n_union} {mode}")
    return stats


def _modes(fixed, stop):
    return [(u, "fixed") for u in fixed] + [(u, "stop") for u in stop]


# ---- a. the half-storage kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_union, mode", _modes(ir.SWEEP, ir.SWEEP_STOP))
def test_half_storage_sweep(monkeypatch, n_union, mode):
    """Every tile count 1 .. 54 (16 ntile - 5 rows), the exact multiples at which the ring depth, the transposition tiles and the template
    change, and 1, 15, 17 rows."""
    _switches(monkeypatch)
    stats = _run_case(n_union, mode, family="half")
    assert stats["blocked"] and stats["half_storage"] and stats["max_union"] == n_union and stats["patches"] == 1, stats


# ---- b. the full-storage kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_union, mode", _modes(ir.FULL, ir.FULL_STOP))
def test_full_storage_by_switch(monkeypatch, n_union, mode):
    """IMCOM_ITER_SYM=0: the three templates (<8> never runs otherwise) and the tails of the eight-tile prefetch."""
    _switches(monkeypatch, IMCOM_ITER_SYM=0)
    stats = _run_case(n_union, mode, family="full")
    assert stats["blocked"] and not stats["half_storage"] and stats["max_union"] == n_union and stats["patches"] == 1, stats


@pytest.mark.parametrize("n_union, mode", _modes(ir.FULL_DEFAULT + (1025,), ir.FULL_DEFAULT + (1025,)))
def test_full_storage_and_fallback_by_size(monkeypatch, n_union, mode):
    """Without a switch: 865, 880 and 1024 rows take the full-storage kernel; 1025 rows are beyond the blocked solver and the per-pixel
    kernel redoes the node."""
    _switches(monkeypatch)
    stats = _run_case(n_union, mode, family="full" if n_union <= 1024 else "per-pixel")
    assert stats["blocked"] == (n_union <= 1024) and not stats["half_storage"] and stats["max_union"] == n_union, stats


# ---- c. the per-pixel kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_union, mode", _modes(ir.PER_PIXEL, ir.PER_PIXEL))
def test_per_pixel_kernel(monkeypatch, n_union, mode):
    """IMCOM_ITER_PER_PIXEL=1 around the ownership edges of its 256 threads (a thread's second row begins at 257 rows of a SELECTION: the
    unions here hold selections on both sides of 256 and 512)."""
    _switches(monkeypatch, IMCOM_ITER_PER_PIXEL=1)
    stats = _run_case(n_union, mode, family="per-pixel")
    assert not stats["blocked"] and not stats["half_storage"], stats


@pytest.mark.parametrize("n_sel", (255, 256, 257, 511, 513) + ir.PER_PIXEL_ONE)
def test_per_pixel_kernel_one_pixel(monkeypatch, n_sel):
    """One output pixel whose SELECTION has exactly n_sel rows (with 16 pixels only the union is exact), up to the kernel's 4096."""
    _switches(monkeypatch, IMCOM_ITER_PER_PIXEL=1)
    for mode in ("fixed",) if n_sel > 513 else ("fixed", "stop"):
        stats = _run_case(n_sel, mode, m_side=(1, 1), family="per-pixel m=1")
        assert not stats["blocked"], stats


def test_per_pixel_kernel_beyond_its_limit(monkeypatch):
    """4097 rows in one disc: the library's error names the limit, and T is untouched by any solve."""
    from pyimcom_amd._lib import ImcomError

    _switches(monkeypatch, IMCOM_ITER_PER_PIXEL=1)
    c = ir.case_for(4097, (1, 1))
    with pytest.raises(ImcomError, match=r"4097 input pixels inside one acceptance disc exceed the limit of 4096") as ei:
        _solve([c], 0.0, ir.MAXITER_FIXED, T_fill=7.0)
    assert (ei.value.T == np.float32(7.0)).all()
    _run_case(255, "fixed", m_side=(1, 1), family="per-pixel after the error")  # the context serves the next call


# ---- d, e. the ragged batch and its sub-batches -----------------------------------------------------------------------------------------
def _ragged(rtol=0.0, maxiter=ir.MAXITER_FIXED):
    return _solve(ir.ragged_batch(), rtol, maxiter)


def _check_ragged(out):
    T, UC, Sg, kp, stats, steps = out
    stamps, refs = ir.ragged_batch(), ir.ragged_reference(0.0, ir.MAXITER_FIXED)
    nonempty = 0
    for s, (c, ref) in enumerate(zip(stamps, refs)):
        if c is None:  # lakernel.py:110-119
            assert np.all(UC[s] == 1) and np.all(Sg[s] == 0) and np.all(kp[s] == 1) and not T[s].any() and not steps[s].any()
            continue
        T_ld, steps_ld, err = ref
        in_patch = np.zeros(c.m, bool)  # pixels of patches that select something: the others are not solved at all (0 steps)
        for pix, un in ir.patch_unions(c.relevant, c.m, c.W):
            nonempty += bool(un.any())
            in_patch[pix] = un.any()
        _check_stamp(c, T[s], UC[s], Sg[s], kp[s], steps[s], T_ld, steps_ld, err, f"ragged stamp {s}", check_steps=in_patch)
        empty_disc = ~c.relevant.any(axis=1)
        assert (empty_disc & in_patch).any() and (~in_patch).any()
        assert not T[s][empty_disc].any() and (steps[s][empty_disc & in_patch] == ir.MAXITER_FIXED).all() and not steps[s][~in_patch].any()
    assert stats["patches"] == nonempty and stats["blocked"] and stats["half_storage"] and stats["max_union"] == 728, stats


def test_ragged_batch(monkeypatch):
    """n = (913, 0, 3), 50 output pixels on a 9 x 6 grid (partial columns, rows and last row), unions of 728, 100, 40, 10, 5 and 0 rows
    in one call: the gather packs by a patch's own tile count, the solver's offsets use the call's largest; a pixel with an empty disc
    keeps its 0 / 0 in its own column."""
    _switches(monkeypatch)
    _check_ragged(_ragged())


@pytest.mark.parametrize("mb, group", [(9, 3), (10, 4)])
def test_sub_batches_are_bit_identical(monkeypatch, mb, group):
    """IMCOM_ITER_BUDGET_MB: the 18 patches of the ragged batch in groups of 3 (six launches; 18 = 6 x 3 leaves no ragged group at this
    size) and of 4 (five launches that cross the stamps, the last of 2 patches).  Selections are indexed by the patch's number in the call,
    sub-matrices and vectors by its number in the group: everything must come out bit for bit as from the single group."""
    ntile = (728 + 15) // 16
    per = (ntile * (ntile + 1) // 2 + 1) * 2048 + 3 * 16 * ntile * 16 * 8  # launch_iter_block: lower tiles + the zero tile, b, x, r
    budget = max(mb << 20, 1024 * 1024 * 8 + 2 * 1024 * 16 * 8)
    assert budget // per == group and (group == 3 or 18 % group)
    _switches(monkeypatch)
    whole = _ragged()
    _switches(monkeypatch, IMCOM_ITER_BUDGET_MB=mb)
    parts = _ragged()
    _check_ragged(parts)
    for a, b in zip(whole[:4] + (whole[5],), parts[:4] + (parts[5],)):
        assert np.array_equal(a, b)
    assert whole[4] == parts[4]


# ---- f. reproducibility -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch, n_union", [(None, 16 * 20 - 5), (None, 16 * 40 - 5), (None, 16 * 52 - 5), ("IMCOM_ITER_SYM", 16 * 17 - 5),
                                             ("IMCOM_ITER_SYM", 16 * 47 - 5), ("IMCOM_ITER_SYM", 16 * 63 - 5), ("IMCOM_ITER_PER_PIXEL", 257)])
def test_same_bits_twice(monkeypatch, switch, n_union):
    """Every template of the three kernels twice: the fixed order of sums the kernel comments promise."""
    _switches(monkeypatch, **({} if switch is None else {switch: 0 if switch == "IMCOM_ITER_SYM" else 1}))
    c = ir.case_for(n_union)
    one, two = _solve([c], ir.RTOL_STOP, ir.MAXITER_STOP), _solve([c], ir.RTOL_STOP, ir.MAXITER_STOP)
    for a, b in zip(one[:4] + (one[5],), two[:4] + (two[5],)):
        assert np.array_equal(a, b)
