"""imcom_build_A / imcom_build_B called directly (C-ABI, device pointers) at their tile, table and pair-code edges, against the
long-double statement of the operation in tests/builder_reference.py -- per element, ``|device - ref| <= K EPS (S + W + |pen|)``
(the constant and its measurement: that module's docstring), and ``==`` for everything that is exact: off-table samples, negative
pair codes, identity and zero padding, symmetry, zero rows and columns of cut grids.  tests/test_builder_reference.py shows (on the
CPU) that the cases contain the edges named here.

Outputs are pre-filled with a sentinel; x / y beyond n[s] are NaN and psf beyond n[s] is a valid index with a table and a penalty
of its own, so that a leak of the padding changes values, not addresses."""

import ctypes as C

import numpy as np
import pytest

from tests import builder_reference as br

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e200


def _dp(t):
    return C.c_void_p(t.data_ptr())


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


def _ctx():
    import torch

    from pyimcom_amd._lib import default_context

    ctx = default_context()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    return ctx


def _common(case):
    import torch

    from pyimcom_amd._lib import TableGeom

    dev = torch.device("cuda:0")
    g = case["geom"]
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    tables = up(case["tables"].ravel())  # exactly ntab * ng * ng doubles
    assert tables.numel() == case["tables"].shape[0] * g.ng * g.ng
    return up, tables, TableGeom(g.nsamp, g.nc, g.dscale, 0.0), np.ascontiguousarray(case["n"], np.int32)


def _build_A(case):
    import torch

    from pyimcom_amd._lib import check, lib

    up, tables, geom, n = _common(case)
    batch, ldn = n.size, case["ldn"]
    x, y, psf, tab, pen = up(case["x"]), up(case["y"]), up(case["psf"]), up(case["pair_tab"]), up(case["pair_pen"])
    A = torch.full((batch, ldn, ldn), SENTINEL, dtype=torch.float64, device=x.device)
    check(lib.imcom_build_A(_ctx().handle, batch, _hp(n), ldn, _dp(x), _dp(y), _dp(psf), _dp(tables), case["tables"].shape[0], C.byref(geom),
                            _dp(tab), _dp(pen), case["npsf_max"], _dp(A)))
    return A.cpu().numpy()


def _build_B(case, ldm):
    import torch

    from pyimcom_amd._lib import check, lib

    up, tables, geom, n = _common(case)
    batch, ldn = n.size, case["ldn"]
    x, y, psf, io, x0, y0 = up(case["x"]), up(case["y"]), up(case["psf"]), up(case["io_tab"]), up(case["out_x0"]), up(case["out_y0"])
    Bt = torch.full((batch, ldn, ldm), SENTINEL, dtype=torch.float64, device=x.device)
    check(lib.imcom_build_B(_ctx().handle, batch, _hp(n), ldn, _dp(x), _dp(y), _dp(psf), _dp(tables), case["tables"].shape[0], C.byref(geom),
                            _dp(io), case["npsf_max"], _dp(x0), _dp(y0), case["n2f"], ldm, _dp(Bt)))
    return Bt.cpu().numpy()


def _within(got, ref, what):
    """Per element inside K EPS (S + W + |pen|); exact where that is zero.  Prints the largest distance in units of the bound."""
    bound = ref.bound()
    err = np.abs(got.astype(br.LD) - ref.val).astype(np.float64)
    units = np.where(err == 0, 0.0, err / np.where(bound == 0, np.finfo(np.float64).tiny, bound))
    print(f"{what}: max |device - ref| / bound = {units.max() if units.size else 0.0:.3f} (bound = {br.K} EPS (S + W + |pen|)), {units.size} elements")
    assert (err <= bound).all(), (what, float(units.max()), np.unravel_index(units.argmax(), units.shape))


def _check_A(case, A, refs):
    ldn = case["ldn"]
    for s, ref in enumerate(refs):
        n, a = int(case["n"][s]), A[s]
        what = f"{case['name']}[{s}] n={n}"
        assert not np.isnan(a).any() and not (a == SENTINEL).any(), what  # all of [ldn][ldn] is written
        assert np.array_equal(a, a.T), what
        pad = np.eye(ldn)
        assert np.array_equal(a[n:], pad[n:]) and np.array_equal(a[:, n:], pad[:, n:]), what  # identity out to ldn
        got = a[:n, :n]
        assert np.array_equal(got[~ref.valid], ref.pen[~ref.valid]), what  # off the table / no table: exactly the pair's penalty
        _within(got, ref, what)


def _check_B(case, Bt, refs, ldm):
    m = case["n2f"] ** 2
    for s, ref in enumerate(refs):
        n, b = int(case["n"][s]), Bt[s]
        what = f"{case['name']}[{s}] n={n} ldm={ldm}"
        assert not np.isnan(b).any() and not (b == SENTINEL).any(), what
        assert not b[n:].any() and not b[:, m:].any(), what  # padding rows and columns are exactly zero
        got = b[:n, :m]
        zero = (ref.S == 0) & (ref.W == 0)
        assert not got[zero].any(), what  # rows and columns off the table: exact zeros
        _within(got, ref, what)


def _A(name):
    return next((c, r) for c, r in br.refs_A() if c["name"] == name)


def _B(name):
    return next((c, r) for c, r in br.refs_B() if c["name"] == name)


# ------------------------------------------------------------------------------------------------ imcom_build_A
@pytest.mark.parametrize("ldn", [256, 200])
def test_build_A_ragged_batch(ldn):
    """n = 0, 1, 15, 16, 17, 127, 128, 129, 200 in one batch, three PSFs interleaved pixel by pixel (the tile order is keyed by a
    tile's first sample only), ldn a multiple of 16 and not: tiles beyond ceil(n / 128) * 128, tiles straddling n, guards at ldn.
    Every stamp alone gives the bits it gives inside the batch."""
    case, refs = _A(f"ragged_ldn{ldn}")
    A = _build_A(case)
    _check_A(case, A, refs)
    for s in range(case["n"].size):
        assert np.array_equal(_build_A(br.alone(case, s))[0], A[s]), s


@pytest.mark.parametrize("P", [3, 8, 9])
def test_build_A_pair_codes(P):
    """Plain, FLIP, SWAP, FLIP|SWAP and negative codes over the ordered pairs of P PSFs on tables without any symmetry, a penalty per
    pair, pixels in scrambled PSF order; the pair table from LDS (P <= 8) and from global memory (P = 9)."""
    case, refs = _A(f"codes_P{P}")
    A = _build_A(case)
    _check_A(case, A, refs)
    for s, ref in enumerate(refs):
        neg = ref.code < 0
        assert neg.any() and np.array_equal(A[s][:40, :40][neg], ref.pen[neg])
        d, rd = np.diagonal(A[s])[:40], np.diagonal(ref.val)  # zero separation + pen(p, p)
        assert (np.abs(d - rd) <= np.diagonal(ref.bound())).all()


def test_build_A_boundary_cells():
    """Separations that put x and, independently, y in cells 3, 4, ng - 6 and ng - 5 (fh = -0.5 exactly among them) for every kind of
    pair: the invalid ones are exactly the penalty, the valid ones inside the bound."""
    case, refs = _A("boundary")
    _check_A(case, _build_A(case), refs)


@pytest.mark.parametrize("ntab", [1, 3])
def test_build_A_end_of_the_table_stack(ntab):
    """Stencils that end on the last element of the table stack -- cell (ng-6, ng-6) of the last table, cell (4, 4) of the flipped last
    table -- among ordinary samples of tile (0, 0), which then runs the guarded row loop as a whole; the same separations on the first
    table fill tile (0, 1), which (ntab = 3) does not."""
    case, refs = _A(f"stack_end_ntab{ntab}")
    _check_A(case, _build_A(case), refs)


# ------------------------------------------------------------------------------------------------ imcom_build_B
@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("n2f", [1, 2, 7, 48])
def test_build_B_small_shapes(n2f, pad):
    """n2f = 1, 2, 7, 48 at dscale = 0.5, stamps of 20, 0 and 7 pixels, ldm = m and m rounded up to 128; two tables, one the last of the
    stack, grids reaching its first and last valid cells and one cell beyond."""
    case, refs = _B(f"small_n2f{n2f}")
    m = n2f * n2f
    ldm = (m + 127) // 128 * 128 if pad else m
    _check_B(case, _build_B(case, ldm), refs, ldm)


def test_build_B_row_loop_tails():
    """n2f = 48: five lanes per column walk the window 15 rows per trip; nrows = 14, 15 and 16 (here), 104, 90 and 76 (small, cut)."""
    case, refs = _B("tails_n2f48")
    _check_B(case, _build_B(case, 48 * 48), refs, 48 * 48)


@pytest.mark.parametrize("name", ["fallback_direct", "fallback_lds"])
def test_build_B_direct_fallback(name):
    """n2f = 48 on a table of side 449: at dscale = 0.125 the 386-row window does not fit and the direct 100-tap form runs; the same
    pixels at dscale = 0.5 take the LDS form."""
    case, refs = _B(name)
    _check_B(case, _build_B(case, 48 * 48), refs, 48 * 48)


@pytest.mark.parametrize("name,pad", [("wide_lds", True), ("wide_direct", False)])
def test_build_B_wide_grid(name, pad):
    """n2f = 257 > 256 threads (the strided x- and y-passes), LDS form (dscale = 32) and direct form (dscale = 8)."""
    case, refs = _B(name)
    m = 257 * 257
    ldm = (m + 127) // 128 * 128 if pad else m
    _check_B(case, _build_B(case, ldm), refs, ldm)


@pytest.mark.parametrize("n2f", [7, 48])
def test_build_B_cut_grids(n2f):
    """Grids leaving the table on the left, right, top, bottom, at a corner, and entirely (in y: no valid row; in x: no valid
    column): the reference's zero rows and columns are exact zeros, the rest is inside the bound."""
    case, refs = _B(f"cut_n2f{n2f}")
    ldm = (n2f * n2f + 127) // 128 * 128
    _check_B(case, _build_B(case, ldm), refs, ldm)
