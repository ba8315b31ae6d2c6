"""The reference of tests/test_gpu_iter_edges.py checked on the host: cg_ld agrees with the oracle's float64 CG and with a direct solve,
every committed case meets the conditions that make a per-element statement possible (exact union sizes: asserted by the builder; cond
below 100; no stopping test within 1e-9 of its threshold, so that NO pixel is excluded from step equality; mixed stop steps inside a
patch), and the bound bites -- a single 16 x 16 tile dropped from the product moves the iterate by more than 1000 bounds."""

import numpy as np
import pytest

from tests import iter_reference as ir

STOP_CASES = sorted(set(ir.SWEEP_STOP) | set(ir.FULL_STOP) | set(ir.FULL_DEFAULT) | {1025} | set(ir.PER_PIXEL))
ALL_16 = sorted(set(ir.SWEEP) | set(ir.FULL) | set(STOP_CASES))


@pytest.mark.parametrize("n_union", [59, 300])
def test_cg_ld_against_the_oracle_and_a_direct_solve(n_union):
    from oracle import oracle as orc

    c = ir.case_for(n_union)
    AA = c.A + c.kappa * np.eye(c.n)
    for a in (0, 5, 15):
        sel = np.nonzero(c.relevant[a])[0]
        As, b = AA[np.ix_(sel, sel)], c.mBhalf[a, sel]
        for k in (3, 8):  # fixed steps
            x, steps, ratios = ir.cg_ld(As, b, 0.0, k)
            xo = orc.conjugate_gradient(As, b.copy(), 0.0, k)
            assert steps == k and len(ratios) == k
            assert np.abs(xo - x.astype(np.float64)).max() <= 1e-13 * np.abs(xo).max()
        x, steps, ratios = ir.cg_ld(As, b, 1e-12, 500)
        assert steps < 500 and ratios[-1] < 1.0 and all(r >= 1.0 for r in ratios[:-1])
        xs = np.linalg.solve(As, b)
        assert np.abs(xs - x.astype(np.float64)).max() <= 1e-10 * np.abs(xs).max()


def test_solve_patchwise_is_the_oracles_wrapper():
    """Same selections, same diagonal, float32(T_ld) against the oracle's float32 T: one float32 rounding apart at the most."""
    from oracle import oracle as orc

    c = ir.case_for(59)
    T, steps, _ = ir.solve_patchwise(c.A, c.kappa, c.mBhalf, c.relevant, ir.RTOL_STOP, ir.MAXITER_STOP)
    osteps = []
    To = orc._iterative_wrapper(c.A + c.kappa * np.eye(c.n), c.mBhalf, c.relevant, ir.RTOL_STOP, ir.MAXITER_STOP, steps=osteps)
    assert np.array_equal(steps, osteps) and np.array_equal(To == 0, T == 0)
    assert (np.abs(To - T) <= 2.0**-23 * np.abs(T)).all()


@pytest.mark.parametrize("n_union", ALL_16)
def test_committed_case_is_well_conditioned(n_union):
    c = ir.case_for(n_union)  # (the builder asserts the union size, the rim's share and min |A| >= 1e-3 max |A|)
    lam = np.linalg.eigvalsh(c.A + c.kappa * np.eye(c.n))
    assert lam[0] > 0 and lam[-1] / lam[0] < 100
    _, steps, _, err = ir.reference(n_union, (4, 4), 0.0, ir.fixed_maxiter(n_union))
    assert (steps == ir.fixed_maxiter(n_union)).all() and err < 1e-10  # (10 ref_err stays far below float32's 2^-24)


@pytest.mark.parametrize("n_union", STOP_CASES)
def test_committed_case_stops_cleanly(n_union):
    """At rtol 1.5e-3: no tested ratio |r| / atol within 1e-9 of 1 (nothing to exclude from step equality), the float64 oracle in both
    index orders takes the long-double run's steps (reference() would otherwise report a distance of order one), 6 to 40 steps and at
    least three distinct stop steps in the patch.  A one-row system ends after one step whatever its condition."""
    _, steps, ratios, err = ir.reference(n_union, (4, 4), ir.RTOL_STOP, ir.MAXITER_STOP)
    flat = np.array([x for r in ratios for x in r])
    assert np.abs(flat - 1.0).min() > 1e-9 and err < 1e-10
    if n_union == 1:
        assert (steps == 1).all()
    else:
        assert steps.min() >= 6 and steps.max() <= 40 and len(set(steps.tolist())) >= 3, steps


def test_single_pixel_cases():
    for n_union in ir.PER_PIXEL_ONE:
        c = ir.case_for(n_union, (1, 1))
        assert c.relevant.sum() == n_union and c.m == 1
        _, steps, _, err = ir.reference(n_union, (1, 1), 0.0, ir.MAXITER_FIXED)
        assert steps[0] == ir.MAXITER_FIXED and err < 1e-10
    for n_union in (255, 256, 257, 511, 513):  # exact selection sizes around the ownership edges of the per-pixel kernel's threads
        c = ir.case_for(n_union, (1, 1))
        assert c.relevant.sum() == n_union
        lam = np.linalg.eigvalsh(c.A + c.kappa * np.eye(c.n))
        assert lam[0] > 0 and lam[-1] / lam[0] < 100
        _, steps, ratios, err = ir.reference(n_union, (1, 1), ir.RTOL_STOP, ir.MAXITER_STOP)
        assert 6 <= steps[0] <= 40 and np.abs(np.array(ratios[0]) - 1.0).min() > 1e-9 and err < 1e-10
        assert ir.reference(n_union, (1, 1), 0.0, ir.MAXITER_FIXED)[3] < 1e-10


def test_ragged_batch_conditions():
    big, none, small = ir.ragged_batch()  # (the builder asserts the patches' unions, the empty discs and the empty patch)
    assert none is None and big.n > 900 and small.n == 3
    for c, ref in zip((big, small), (ir.ragged_reference(0.0, ir.MAXITER_FIXED)[0], ir.ragged_reference(0.0, ir.MAXITER_FIXED)[2])):
        T, steps, err = ref
        assert np.isfinite(T).all() and (steps == ir.MAXITER_FIXED).all() and err < 1e-10
        assert not T[c.relevant.sum(axis=1) == 0].any()
    lam = np.linalg.eigvalsh(big.A + big.kappa * np.eye(big.n))
    assert lam[0] > 0 and lam[-1] / lam[0] < 100


@pytest.mark.parametrize("n_union", [208, 720, 1024])
@pytest.mark.parametrize("which", ["first_off_diagonal", "last_row_first", "transposed_use_only"])
def test_a_dropped_tile_is_far_outside_the_bound(n_union, which):
    """One 16 x 16 tile of the patch's sub-matrix AU = AA[U][U] left out of the product q = AU p: tile (1, 0) with its mirror image (a
    stored lower tile serves both), tile (ntile - 1, 0) with its mirror image, or the transposed use of tile (1, 0) alone (q_0 += T^T p_1).
    The six-step iterate of some pixel must move by more than 1000 bounds: the device assertions can fail."""
    c = ir.case_for(n_union)
    T, _, _, err = ir.reference(n_union, (4, 4), 0.0, ir.MAXITER_FIXED)
    U = np.nonzero(c.relevant.any(axis=0))[0]
    ntile = (U.size + 15) // 16
    I, K = (ntile - 1, 0) if which == "last_row_first" else (1, 0)
    pos = np.full(c.n, -1)
    pos[U] = np.arange(U.size)
    AA = c.A + c.kappa * np.eye(c.n)
    worst = 0.0
    for a in range(c.m):
        sel = np.nonzero(c.relevant[a])[0]
        tile = pos[sel] // 16
        As = AA[np.ix_(sel, sel)].copy()
        if which != "transposed_use_only":
            As[np.ix_(tile == I, tile == K)] = 0.0
        As[np.ix_(tile == K, tile == I)] = 0.0
        x, _, _ = ir.cg_ld(As, c.mBhalf[a, sel], 0.0, ir.MAXITER_FIXED)
        worst = max(worst, (np.abs(x.astype(np.float64) - T[a, sel]) / ir.bound(T[a, sel], err)).max())
    assert worst > 1000.0, worst
