"""tests/builder_reference.py checked on its own (CPU only): the long-double reference is pinned by the float64 oracle and by the
reference's own outputs (tests/golden/interp.npz), the tolerance constant of tests/test_gpu_builder_edges.py is measured here, and
the generated cases are shown to contain the edges they were written for -- from the reference's own cell indices, so that an edit
of the generators cannot lose one silently."""

import numpy as np
import pytest

from oracle import oracle as orc
from tests import builder_reference as br


def _units(got, ref):
    """Distance of float64 ``got`` from the reference in units of EPS * (S + W + |pen|); 0 where both are exactly equal."""
    scale = ref.bound(1.0)
    err = np.abs(got.astype(br.LD) - ref.val).astype(np.float64)
    assert not (err[scale == 0] != 0).any()
    return np.where(err == 0, 0.0, err / np.where(scale == 0, 1.0, scale))


def test_weights_vs_golden(golden):
    g = golden("getw")
    w = br.getw(g["fh"])
    assert np.abs(w - g["w"]).max() <= 4 * br.EPS  # |w| <= 1.3: the float64 Horner form is a few eps from the long double one
    assert np.abs(w.sum(-1) - 1).max() < 1e-7  # the weights of a constant


def test_reference_vs_oracle_and_K():
    """ref_A / ref_Bt against oracle.stamp_system on every generated case.  The largest distance in units of EPS * (S + W + |pen|) is
    what K_ORACLE records; K = 4 K_ORACLE is the device's bound."""
    worst = {"A": 0.0, "B": 0.0}
    count = {"A": 0, "B": 0}
    for case, refs in br.refs_A():
        for s, ref in enumerate(refs):
            x, y, psf, tables, g, tab, pen = br.stamp_A(case, s)
            if x.size == 0:
                assert ref.val.shape == (0, 0)
                continue
            A, _ = orc.stamp_system(g, x, y, psf, tables, tab, pen, np.zeros(tab.shape[0], np.int32), 0.0, 0.0, 1)
            u = _units(A, ref)
            assert np.array_equal(A[~ref.valid], ref.pen[~ref.valid])  # off the table or no table: the penalty itself
            assert np.array_equal(ref.val[~ref.valid].astype(np.float64), ref.pen[~ref.valid])
            worst["A"], count["A"] = max(worst["A"], u.max()), count["A"] + int(np.triu(ref.valid).sum())
    for case, refs in br.refs_B():
        for s, ref in enumerate(refs):
            x, y, psf, tables, g, io, x0, y0, n2f = br.stamp_B(case, s)
            if x.size == 0:
                assert ref.val.shape == (0, n2f * n2f)
                continue
            P = io.size
            _, Bt = orc.stamp_system(g, x, y, psf, tables, np.full((P, P), -1, np.int32), np.zeros((P, P)), io, x0, y0, n2f)
            u = _units(Bt, ref)
            assert np.array_equal(Bt == 0, ref.S == 0)  # the zero rows and columns of cut grids
            worst["B"], count["B"] = max(worst["B"], u.max()), count["B"] + int((ref.S != 0).sum())
    print("oracle distance from the long-double reference, units of EPS (S + W + |pen|):", worst, "samples:", count)
    assert max(worst.values()) <= br.K_ORACLE
    assert max(worst.values()) > br.K_ORACLE / 2  # (the recorded figure is the measured one, not a loose guess)
    assert br.K == 4 * br.K_ORACLE


def test_reference_vs_golden_interp(golden):
    """The reference's own outputs (tests/golden/interp.npz): scattered points on two layers and on a 40 x 37 table, and the
    separable grid."""
    g = golden("interp")
    for tabs, x, y, f in ((g["infunc"], g["x"], g["y"], g["f_scatter"]), (g["infunc_b"], g["xb"], g["yb"], g["f_scatter_b"])):
        for layer, fl in zip(tabs, f):
            val, S, W, valid, _, _ = br.interp_points(layer, x, y)
            assert valid.any() and (np.abs(fl[valid] - val[valid]) <= br.K_ORACLE * br.EPS * (S + W)[valid]).all()
    assert np.array_equal(g["f_scatter"][0] == -7.0, ~br.interp_points(g["infunc"][0], g["x"], g["y"])[3])  # untouched off the grid
    for xp, yp, f in zip(g["xpos"], g["ypos"], g["f_grid"]):
        val, S, W, _, _ = br.interp_grid(g["infunc"][0], xp, yp)
        assert (np.abs(f.reshape(val.shape) - val) <= br.K_ORACLE * br.EPS * (S + W)).all() and np.array_equal(f.reshape(val.shape) == 0, S == 0)


def test_positions_are_exact():
    """Every position is a multiple of 1/64 and every dscale a power of two: the cell decisions do not depend on the arithmetic."""
    for case in br.cases_A() + br.cases_B():
        for s, n in enumerate(case["n"]):
            v = np.concatenate([case["x"][s, :n], case["y"][s, :n]]) * 64
            assert np.array_equal(v, np.round(v)) and np.isnan(case["x"][s, n:]).all() and np.isnan(case["y"][s, n:]).all()
            assert (case["psf"][s] >= 0).all() and (case["psf"][s] < case["npsf_max"]).all()
        assert np.log2(case["geom"].dscale) % 1 == 0 and case["geom"].nc % 1 == 0
        assert case["tables"].shape[1:] == (case["geom"].ng,) * 2
        t = case["tables"]
        assert not t[:, :6].any() and not t[:, -6:].any() and not t[:, :, :6].any() and not t[:, :, -6:].any()  # the zero border


def _near_end(ref, ntab, ng):
    """Samples whose stencil ends on the last element of the table stack (build_A_kernel's near_end): on the last table, cell
    (ng-6, ng-6) unflipped, cell (4, 4) flipped."""
    code = ref.code
    last = ref.valid & (code >= 0) & ((code & br.PAIR_MASK) == ntab - 1)
    flip = (code & br.PAIR_FLIP) != 0
    return (last & ~flip & (ref.xi == ng - 6) & (ref.yi == ng - 6)), (last & flip & (ref.xi == 4) & (ref.yi == 4))


def test_cases_A_cover_the_edges():
    refs = {c["name"]: (c, r) for c, r in br.refs_A()}
    assert set(refs) == {"ragged_ldn256", "ragged_ldn200", "codes_P3", "codes_P8", "codes_P9", "boundary", "stack_end_ntab1", "stack_end_ntab3"}
    # ragged batch: the issue's sizes, three interleaved PSFs, both leading dimensions
    for name, ldn in (("ragged_ldn256", 256), ("ragged_ldn200", 200)):
        c, r = refs[name]
        assert tuple(c["n"]) == (0, 1, 15, 16, 17, 127, 128, 129, 200) and c["ldn"] == ldn
        for s, n in enumerate(c["n"]):
            assert np.array_equal(c["psf"][s, :n], np.arange(n) % 3) and (c["psf"][s, n:] == 3).all()
        assert any((~x.valid & (x.code >= 0)).any() for x in r) and any((x.code < 0).any() for x in r)
    # pair codes: every kind among the samples i < j, each with a penalty of its own; the LDS / global boundary of the pair table
    for P in (3, 8, 9):
        c, r = refs[f"codes_P{P}"]
        assert c["npsf_max"] == P and tuple(c["n"]) == (40, 40)
        for s, x in enumerate(r):
            iu = np.triu_indices(40, 1)
            code = x.code[iu]
            for kind in (0, br.PAIR_FLIP, br.PAIR_SWAP, br.PAIR_FLIP | br.PAIR_SWAP):
                assert (x.valid[iu] & (code >= 0) & ((code & ~br.PAIR_MASK) == kind)).any(), (P, s, kind)
            assert (code < 0).any()
            assert x.valid[iu][code >= 0].all()  # every sample with a table is on it: its value depends on the table
            assert np.unique(c["pair_pen"][s]).size == P * P
            assert len(set(zip(c["psf"][s, :40][iu[0]], c["psf"][s, :40][iu[1]]))) == P * P  # every ordered pair occurs
            assert not np.array_equal(c["psf"][s, :40], np.sort(c["psf"][s, :40]))  # scrambled
    # boundary cells, x and y independently, on valid and invalid sides, for every kind of pair; fh = -0.5 exactly
    c, (x,) = refs["boundary"]
    ng = c["geom"].ng
    for kind in (0, br.PAIR_FLIP, br.PAIR_SWAP, br.PAIR_FLIP | br.PAIR_SWAP):
        k = (x.code >= 0) & ((x.code & ~br.PAIR_MASK) == kind)
        for cell, ok in ((3, False), (4, True), (ng - 6, True), (ng - 5, False)):
            assert (k & (x.xi == cell) & (x.yi > 4) & (x.yi < ng - 6) & (x.valid == ok)).any(), (kind, cell)
            assert (k & (x.yi == cell) & (x.xi > 4) & (x.xi < ng - 6) & (x.valid == ok)).any(), (kind, cell)
    px, py, g = c["x"][0, :39], c["y"][0, :39], c["geom"]
    dx, dy = br.position(px[0], px[1:], g), br.position(py[0], py[1:], g)
    for d in (3.0, 4.0, ng - 6.0, ng - 5.0):
        assert (dx == d).any() and (dy == d).any()  # fh = -0.5 exactly
    # end of the stack
    for ntab in (1, 3):
        c, (x,) = refs[f"stack_end_ntab{ntab}"]
        assert c["tables"].shape[0] == ntab
        plain, flipped = _near_end(x, ntab, ng)
        t00 = (slice(0, 16), slice(0, 16))
        assert plain[t00][0].any() and flipped[t00][0].any()  # the anchor's row of tile (0, 0)
        assert not (plain | flipped)[t00].all()  # among ordinary samples
        if ntab == 3:  # the same separations on the first table, in a tile of their own: the unguarded control
            t01 = (slice(0, 16), slice(16, 32))
            assert not (plain | flipped)[t01].any()
            first = x.valid & ((x.code & br.PAIR_MASK) == 0)
            flip = (x.code & br.PAIR_FLIP) != 0
            assert (first & ~flip & (x.xi == ng - 6) & (x.yi == ng - 6))[t01].any() and (first & flip & (x.xi == 4) & (x.yi == 4))[t01].any()
    # over all cases: the two corner samples, and cells 3, 4, ng-6, ng-5 in each axis
    every = [x for _, r in br.refs_A() for x in r]
    for cell in (3, 4, ng - 6, ng - 5):
        assert any(((x.code >= 0) & (x.xi == cell)).any() for x in every) and any(((x.code >= 0) & (x.yi == cell)).any() for x in every)
    # the diagonal: zero separation sits at the start of the centre cell (fh = -0.5), where D5512 returns the sample itself
    c, r = refs["codes_P3"]
    d = np.diagonal(r[0].val).astype(np.float64) - np.diagonal(r[0].pen)
    code = np.diagonal(r[0].code)
    for i in np.flatnonzero(code >= 0):
        at = ng - 1 - 32 if code[i] & br.PAIR_FLIP else 32  # np.flip maps sample 32 to ng - 1 - 32
        assert abs(d[i] - c["tables"][code[i] & br.PAIR_MASK][at, at]) < 1e-6
    assert (code >= 0).sum() >= 20


def _grids(case, refs):
    """Per pixel of a B case: (ref, pixel index, validity of its columns, of its rows, nrows)."""
    ng = case["geom"].ng
    for ref in refs:
        for i in range(ref.xi.shape[0]):
            vx, vy = (ref.xi[i] >= 4) & (ref.xi[i] < ng - 5), (ref.yi[i] >= 4) & (ref.yi[i] < ng - 5)
            yield ref, i, vx, vy, br.grid_rows(ref.yi[i], ng)[2]


def test_cases_B_cover_the_edges():
    refs = {c["name"]: (c, r) for c, r in br.refs_B()}
    assert set(refs) == {f"small_n2f{k}" for k in (1, 2, 7, 48)} | {"cut_n2f7", "cut_n2f48", "tails_n2f48", "fallback_direct", "fallback_lds",
                                                                     "wide_lds", "wide_direct"}
    # which form runs: grid_lds's arithmetic restated (br.grid_lds_rows)
    assert br.grid_lds_rows(48, 0.5) == 107 and br.grid_lds_rows(48, 0.125) == 234 and br.grid_lds_rows(257, 32.0) == 21 and br.grid_lds_rows(257, 8.0) == 26
    form = {}
    for name, (c, r) in refs.items():
        max_rows = br.grid_lds_rows(c["n2f"], c["geom"].dscale)
        form[name] = {"direct" if nrows > max_rows else "lds" for _, _, _, _, nrows in _grids(c, r) if nrows}
    assert form["fallback_direct"] == {"direct"} and form["wide_direct"] == {"direct"}
    assert all(f == {"lds"} for name, f in form.items() if name not in ("fallback_direct", "wide_direct")), form
    a, b = refs["fallback_direct"][0], refs["fallback_lds"][0]
    assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["y"], b["y"]) and a["tables"] is b["tables"] and a["n2f"] == b["n2f"] == 48
    assert a["tables"].shape[1] == 449 and refs["wide_lds"][0]["n2f"] == 257 and tuple(refs["wide_lds"][0]["n"]) == (3,)
    # the x-pass walks 3 nlane rows per trip: the residues 0, 1 and 3 nlane - 1 at n2f = 48 (nlane = 5), in the LDS form
    res = {nrows % 15 for name in ("small_n2f48", "cut_n2f48", "tails_n2f48") for _, _, _, _, nrows in _grids(*refs[name]) if nrows}
    assert {0, 1, 14} <= res, res
    assert {nrows for _, _, _, _, nrows in _grids(*refs["tails_n2f48"])} == {14, 15, 16}  # by the fraction of the offset alone
    # small shapes: three stamps, one empty; two tables, one of them the last, whose last and first valid cells are reached
    for n2f in (1, 2, 7, 48):
        c, r = refs[f"small_n2f{n2f}"]
        ng = c["geom"].ng
        assert tuple(c["n"]) == (20, 0, 7) and c["geom"].dscale == 0.5 and c["ldn"] > 20
        last = c["tables"].shape[0] - 1
        assert any((x.tab == last).any() and (x.tab != last).any() for x in r if x.tab.size)
        for cell in (4, ng - 6):
            assert any((x.yi[x.tab == last] == cell).any() for x in r) and any((x.xi[x.tab == last] == cell).any() for x in r)
    # cut on each side, at a corner, and entirely off; both for the LDS and for the direct form
    for name in ("cut_n2f7", "cut_n2f48", "fallback_direct", "wide_lds", "wide_direct"):
        c, r = refs[name]
        ng = c["geom"].ng
        sides = set()
        for ref, i, vx, vy, nrows in _grids(c, r):
            part_x, part_y = vx.any() and not vx.all(), vy.any() and not vy.all()
            if part_x and vy.any():
                sides.add("left" if (ref.xi[i][~vx] < 4).all() else "right")
            if part_y and vx.any():
                sides.add("top" if (ref.yi[i][~vy] < 4).all() else "bottom")
            if part_x and part_y:
                sides.add("corner")
            if not vy.any():
                sides.add("off_y")
                assert not ref.S[i].any() and not ref.val[i].any()
            if not vx.any():
                sides.add("off_x")
                assert not ref.S[i].any()
        if name.startswith("cut"):
            assert sides == {"left", "right", "top", "bottom", "corner", "off_y", "off_x"}, (name, sides)
        else:
            assert len(sides & {"left", "right", "top", "bottom"}) >= 2, (name, sides)
    # cells 3, 4, ng-6 and ng-5 in each axis
    for name in ("small_n2f7", "small_n2f48", "cut_n2f48"):
        c, r = refs[name]
        ng = c["geom"].ng
        for cell in (3, 4, ng - 6, ng - 5):
            assert any((x.xi == cell).any() for x in r) and any((x.yi == cell).any() for x in r), (name, cell)
