"""pyimcom_amd.reportstats on the device (csrc/quantiles.hip) against numpy and against the reference's own outputs
(tests/golden/reportstats.npz).  Every comparison is exact equality (np.array_equal: -0.0 equals 0.0 there; NaN positions are compared on
their own): order statistics and integer counts have one right value, and the scalar steps are numpy's own on the host."""

import numpy as np
import pytest

from tests.test_reportstats_host import G, golden_frames

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNKS = (1, 63, 64, 65, 4097, 513, 2000)  # 7 chunks of unequal sizes around a wave, a workgroup and a grid


def same(a, b):
    """Equal values where neither is NaN, NaN in the same places."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def ranks26(n):
    """26 ranks of n values: 0 and n - 1 and pairs of neighbours in between."""
    r = []
    for k in range(13):
        p = int((n - 1) * k / 12)
        r += [p, min(p + 1, n - 1)]
    return np.asarray(r, dtype=np.int64)


def select(chunks, ranks, dtype=np.float32, **kw):
    """Order statistics of the concatenation of ``chunks`` (one segment) through the pass loop."""
    from pyimcom_amd.reportstats import StreamingQuantiles

    sq = StreamingQuantiles(1, dtype, n_ranks=len(ranks), **kw)
    out = sq.run(lambda s: [s.add(c) for c in chunks], np.asarray(ranks)[None, :])
    total, nans = sq.counts()
    sq.close()
    return out[0], int(total[0]), int(nans[0])


def test_chunking_and_ranks():
    rng = np.random.default_rng(11)
    chunks = [rng.standard_normal(n).astype(np.float32) for n in CHUNKS]
    allv = np.concatenate(chunks)
    ranks = ranks26(allv.size)
    assert ranks[0] == 0 and ranks[-1] == allv.size - 1 and len(ranks) == 26
    want = np.sort(allv)[ranks]
    got, total, nans = select(chunks, ranks)
    assert np.array_equal(got, want) and got.dtype == np.float32 and (total, nans) == (allv.size, 0)
    rev, _, _ = select(chunks[::-1], ranks)
    one, _, _ = select([allv], ranks)
    assert got.tobytes() == rev.tobytes() == one.tobytes()


def test_strided_views_are_read_in_place():
    import torch

    frame = G["frames_0_0"][0]
    assert frame.shape == (40, 40)
    t = torch.as_tensor(frame, device=DEV)
    for d in (4, 0):
        view = t[d:40 - d, d:40 - d]
        assert view.stride(0) == 40 and view.data_ptr() == t.data_ptr() + 4 * (40 * d + d)
        crop = frame[d:40 - d, d:40 - d].ravel()
        ranks = ranks26(crop.size)
        got, total, _ = select([view], ranks)
        assert np.array_equal(got, np.sort(crop)[ranks]) and total == crop.size


def test_ties_and_specials():
    f = np.float32
    cases = {
        "all_equal": np.full(1000, 2.5, dtype=f),
        "two_values": np.concatenate([np.full(300, -1.0, dtype=f), np.full(700, 3.0, dtype=f)]),
        "nans": np.concatenate([np.arange(90, dtype=f), np.full(10, np.nan, dtype=f)]),
        "inf_denormal_zero": np.array([np.inf, -np.inf, 1e-45, -1e-45, 1e-40, 0.0, -0.0, 0.0, -0.0, 1.0, -1.0, np.inf], dtype=f),
        "n2": np.array([7.0, -7.0], dtype=f),
    }
    rng = np.random.default_rng(3)
    for name, a in cases.items():
        a = rng.permutation(a)
        n = a.size
        ranks = np.unique(np.concatenate([ranks26(n), [299, 300] if name == "two_values" else [n - 1], [89, 90, 95] if name == "nans" else [0]]))
        got, total, nans = select([a[: n // 2], a[n // 2:]], ranks)
        want = np.sort(a)[ranks]  # (numpy sorts NaNs last too)
        assert same(got, want), name
        assert (total, nans) == (n, int(np.isnan(a).sum())), name
    got, _, _ = select([cases["two_values"]], [299, 300])
    assert list(got) == [-1.0, 3.0]  # the ranks on both sides of the step
    got, _, _ = select([cases["nans"]], [89, 90])
    assert got[0] == 89.0 and np.isnan(got[1])  # the last number, the first NaN
    got, _, _ = select([cases["inf_denormal_zero"]], np.arange(12))
    # sorted: -inf, -1, -1e-45, the four zeros, 1e-45, 1e-40, 1, inf, inf; -0.0 and 0.0 are one value and come back as 0.0
    assert np.array_equal(got, np.sort(cases["inf_denormal_zero"])) and got[2] == np.float32(-1e-45) and got[7] == np.float32(1e-45)
    assert not np.signbit(got[3:7]).any() and (got[3:7] == 0).all()


def test_many_live_prefixes_tile_the_groups():
    # 26 ranks in 26 different first digits (sign, exponent, two mantissa bits): powers of 4 from 4^-13 to 4^12, 40 values around each
    rng = np.random.default_rng(8)
    base = 4.0 ** np.arange(-13, 13)
    a = (base[:, None] * rng.uniform(1.0, 1.2, size=(26, 40))).astype(np.float32)
    digits = (a[:, 0].view(np.uint32) >> 21)
    assert np.unique(digits).size == 26
    ranks = np.arange(26) * 40 + rng.integers(0, 40, size=26)
    flat = rng.permutation(a.ravel())
    got, _, _ = select([flat[:500], flat[500:]], ranks)
    assert np.array_equal(got, np.sort(flat)[ranks])
    got64, _, _ = select([flat[:500].astype(np.float64), flat[500:].astype(np.float64)], ranks, dtype=np.float64)
    assert np.array_equal(got64, np.sort(flat.astype(np.float64))[ranks])


@pytest.mark.parametrize("ids_dtype", [np.uint8, np.int32])
def test_many_segments(ids_dtype):
    from pyimcom_amd.reportstats import StreamingQuantiles

    rng = np.random.default_rng(21)
    S, n = 64, 30000
    ids = rng.integers(0, S, size=n)
    ids[ids == 17] = 18  # segment 17 stays empty
    ids[:5] = 63
    vals = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, size=n)).astype(np.float32)
    vals[rng.integers(0, n, size=50)] = np.nan
    counts = np.bincount(ids, minlength=S)
    assert counts[17] == 0 and np.unique(counts).size > 20
    R_ = 8
    ranks = np.stack([np.linspace(0, max(c - 1, 0), R_).astype(np.int64) for c in counts])
    sq = StreamingQuantiles(S, np.float32, n_ranks=R_)
    cut = (0, 1, 7000, 7001, n)
    got = sq.run(lambda s: [s.add(vals[a:b], segment_ids=ids[a:b].astype(ids_dtype)) for a, b in zip(cut, cut[1:])], ranks)
    total, nans = sq.counts()
    assert np.array_equal(total, counts) and total[17] == 0 and np.isnan(got[17]).all()
    for s in range(S):
        if counts[s]:
            v = vals[ids == s]
            assert nans[s] == np.isnan(v).sum()
            assert same(got[s], np.sort(v)[ranks[s]]), s
    # an id outside the segments fails the pass at its end; the accumulator is usable after reset
    from pyimcom_amd._lib import ImcomError

    sq.reset()
    sq.add(vals[:10], segment_ids=np.full(10, 64 if ids_dtype == np.uint8 else -1, dtype=ids_dtype))
    with pytest.raises(ImcomError, match="segment ids"):
        sq.end_pass()
    sq.close()


def test_counts_above_2_to_the_32():
    from pyimcom_amd.reportstats import StreamingQuantiles

    big = 5_000_000_000
    neg, pos = -np.arange(1, 1001, dtype=np.float32), np.arange(1, 1001, dtype=np.float32)
    ranks = np.array([[0, 999, 1000, 1000 + big // 2, 1000 + big - 1, 1000 + big, 1999 + big, 500, 1500 + big]], dtype=np.int64)
    sq = StreamingQuantiles(1, np.float32, n_ranks=ranks.shape[1])

    def feed(s):
        s.add(pos)
        s.add_constant(0, 0.0, big)
        s.add(neg)

    got = sq.run(feed, ranks)[0]
    total, nans = sq.counts()
    sq.close()
    assert total[0] == big + 2000 and nans[0] == 0
    # closed form: ranks 0 .. 999 are -1000 .. -1, the next `big` are 0, then 1 .. 1000
    assert list(got) == [-1000.0, -1.0, 0.0, 0.0, 0.0, 1.0, 1000.0, -500.0, 501.0]


def test_pass_mismatch_raises_and_reset_recovers():
    from pyimcom_amd._lib import ImcomError
    from pyimcom_amd.reportstats import StreamingQuantiles

    rng = np.random.default_rng(4)
    a = rng.standard_normal(5000).astype(np.float32)
    ranks = ranks26(a.size)[None, :]
    sq = StreamingQuantiles(1, np.float32, n_ranks=26)
    sq.add(a)
    assert sq.end_pass() == 2
    sq.set_ranks(ranks)
    sq.add(a[:-1])  # one element fewer than pass 1
    with pytest.raises(ImcomError) as e:
        sq.end_pass()
    assert e.value.status == -1 and "4999" in str(e.value) and "5000" in str(e.value)
    sq.add(a)  # the failed pass has not happened: it can be fed again
    assert sq.end_pass() == 1
    sq.add(a)
    assert sq.end_pass() == 0
    assert np.array_equal(sq.order_statistics()[0], np.sort(a)[ranks[0]])
    sq.reset()
    b = a[:100] * 2
    assert np.array_equal(sq.run(lambda s: s.add(b), np.array([[0, 50, 99]])), np.sort(b)[[0, 50, 99]][None, :])
    sq.close()


def test_float64_route_takes_six_passes():
    from pyimcom_amd.reportstats import StreamingQuantiles

    rng = np.random.default_rng(6)
    a = rng.standard_normal(3001) * 10.0 ** rng.integers(-200, 200, size=3001)
    a[::500] = np.nan
    a[1::500] = -0.0
    sq = StreamingQuantiles(1, np.float64, n_ranks=26)
    assert sq.passes == 6
    ranks = ranks26(a.size)
    got = sq.run(lambda s: [s.add(a[:1000]), s.add(a[1000:].reshape(-1, 1))], ranks[None, :])[0]
    sq.close()
    assert got.dtype == np.float64 and same(got, np.sort(a)[ranks])
    assert np.isnan(got[-1])


# ---- rings ----
def ring_table(starmap, x, y, rpix, **kw):
    from pyimcom_amd.reportstats import dynrange_tables

    return dynrange_tables([dict(starmap=starmap, x=x, y=y, **kw)], rpix, int(G["bd"]))


def test_rings_equal_the_golden_table_and_counts():
    t = ring_table(G["starmap"], G["x"], G["y"], int(G["rpix"]))["dynrange"]
    assert np.array_equal(t[:, 0], np.arange(int(G["rpix"]))) and np.array_equal(t[:, 1], G["ring_counts"])
    assert np.array_equal(t[:, 2:].astype(np.float32), G["ring_percentiles"]) and np.array_equal(t[:, 2:], G["ring_percentiles"].astype(np.float64))
    text = "".join(f"{j:3d} {int(t[j, 1]):8d}" + "".join(f" {np.float32(v):12.5E}" for v in t[j, 2:]) + "\n" for j in range(t.shape[0]))
    assert text == str(G["outst"])


def test_ring_membership_at_exact_squares_edges_and_overlaps():
    from pyimcom_amd.reportstats import StreamingQuantiles
    from tests import reportstats_reference as R

    rng = np.random.default_rng(9)
    n, rpix = 64, 11
    frame = rng.standard_normal((n, n)).astype(np.float32)
    # integer and half-integer offsets (3-4-5, 6-8-10, 5-12-13 halves), a box clipped at each edge, a corner, off the frame, overlapping
    x = np.array([20.0, 40.5, 0.0, 63.0, 30.5, 31.0, 0.5, -20.0, 80.0, 33.0, 36.5, 63.9])
    y = np.array([20.0, 20.5, 30.0, 31.5, 0.0, 63.0, 0.5, 30.0, 30.0, 44.0, 45.5, 63.9])
    want = R.ring_values(frame, x, y, rpix)
    assert sum(v.size for v in R.ring_values(frame, x[7:9], y[7:9], rpix)) == 0
    sq = StreamingQuantiles(rpix, np.float32, n_ranks=3)
    counts = np.array([v.size for v in want])
    ranks = np.stack([[0, c // 2, c - 1] for c in counts])
    got = sq.run(lambda s: s.add_star_rings(frame, x, y, rpix), ranks)
    total, _ = sq.counts()
    sq.close()
    assert np.array_equal(total, counts)
    assert np.array_equal(got, np.stack([np.sort(v)[r] for v, r in zip(want, ranks)]))
    # a position the reference's int16 cannot hold fails the pass
    from pyimcom_amd._lib import ImcomError

    sq = StreamingQuantiles(rpix, np.float32, n_ranks=3)
    sq.add_star_rings(frame, np.array([1e6]), np.array([5.0]), rpix)
    with pytest.raises(ImcomError, match="star positions"):
        sq.end_pass()
    sq.close()


# ---- histograms of coded maps ----
@pytest.mark.parametrize("name", ["sigma", "neff"])
def test_coded_map_histograms_equal_the_golden(name):
    import torch

    from pyimcom_amd import reportstats as RS

    codes, bels, bd = G[name], float(G[f"{name}_bels"]), int(G["bd"])
    assert codes.dtype == (np.int16 if name == "sigma" else np.uint16)
    crop = codes[bd:-bd, bd:-bd]
    ext = (-32768, 32767) if name == "sigma" else (0, 65535)
    assert all((crop == e).any() for e in ext)  # the extreme codes are inside the crop
    allc = RS._all_codes(codes.dtype)
    with np.errstate(all="ignore"):
        vals = 10 ** (0.5 * bels * allc) if name == "sigma" else 10 ** (bels * allc * int(G["nscale"]))
    table = RS.code_bin_table(vals, 0.02 if name == "sigma" else 0.1, 100)
    want, tot = G["countnoise" if name == "sigma" else "countneff"][:, 1], G["totals"][:2] if name == "sigma" else G["totals"][2:]
    t = torch.as_tensor(codes.view(np.int16), device=DEV)
    t = t.view(torch.uint16) if name == "neff" else t
    for arg in (crop, t[bd:-bd, bd:-bd]):  # a numpy array by upload, a device view in place
        h = RS.coded_map_histogram(arg, table, 100)
        assert h.dtype == np.int64 and np.array_equal(h[:100], want) and h[100] == tot[1]


# ---- end to end ----
def test_layer_percentiles_end_to_end():
    import torch

    from pyimcom_amd.reportstats import LAYER_PCTILES, layer_percentiles
    from tests import reportstats_reference as R

    frames = golden_frames()
    on_device = {k: torch.as_tensor(v, device=DEV) for k, v in frames.items()}
    on_device[R.MISSING] = None
    for f in (on_device, frames):
        pc = layer_percentiles(f, R.NS, R.D, R.NBLOCK, LAYER_PCTILES)
        assert pc.dtype == np.float32 and pc.shape == G["pcarray"].shape and np.array_equal(pc, G["pcarray"])


def test_dynrange_tables_end_to_end():
    import torch

    sig = (torch.as_tensor(G["sigma"], device=DEV), float(G["sigma_bels"]))
    neff = (G["neff"], float(G["neff_bels"]))
    out = ring_table(torch.as_tensor(G["starmap"], device=DEV), G["x"], G["y"], int(G["rpix"]), sigma=sig, neff=neff)
    assert np.array_equal(out["countnoise"], G["countnoise"]) and np.array_equal(out["countneff"], G["countneff"])
    tn, tn_gt, te, te_gt = G["totals"]
    assert out["noise_header"] == (np.amax(G["countnoise"][:, 1]), 100 * tn_gt / tn)
    assert out["neff_header"] == (np.amax(G["countneff"][:, 1]), 100 * te_gt / te)
    assert np.array_equal(out["dynrange"][:, 1], G["ring_counts"]) and np.array_equal(out["dynrange"][:, 2:], G["ring_percentiles"].astype(np.float64))


def test_block_maps_hand_out_views():
    import torch

    from pyimcom_amd.block import BlockMaps

    bm = BlockMaps(4, 8, 2, 3, 1, device=DEV)
    frames = bm.report_views(pad=3)
    assert frames.shape[0] == 3 and frames.shape[1] == frames.shape[2] == bm.nside - 2 * (bm.fade + 3)
    assert frames.data_ptr() == bm.out_map[0][:, bm.fade + 3:, bm.fade + 3:].data_ptr() and frames.stride(1) == bm.nside
