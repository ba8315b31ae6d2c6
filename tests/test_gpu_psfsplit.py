"""PSFSPLIT's coaddition stage on the device: wide overlap tables (imcom_psf_overlap_wide, imcom_psf_overlap_spectra_wide), affine sampling
positions (imcom_affine_positions), the A / B builders on wide tables and the Block seam with ``psfsplit=True``, against the reference's
own outputs (tests/golden/psfsplit.npz) and the numpy restatement pinned to them (tests/psfsplit_reference.py).

Bounds are those the unsplit path is held to for the same quantity: tables 2e-13 of the largest entry (tests/test_gpu_stamps.py::
test_psf_overlap_golden, tests/test_gpu_psfs.py: mixed radix, windows), 5e-13 and C to 1e-12 through PSFGroupTables with amp_penalty
(test_amp_penalty_tables_golden), sampled PSFs 1e-13 (test_sample_psf_golden), A and B 1e-13 of the largest entry (tests/parity.py), block
maps as tests/test_gpu_refblock.py::test_block_seam_whole_block_vs_oracle."""

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TAB = 2e-13  # |d table| <= TAB * max |table|


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


def _sizes(g, tag):
    _, oversamp, ns, nfft, ntab = (int(v) for v in g[f"{tag}_pars"])
    return oversamp, ns, nfft, ntab


def _wide_from_psfs(p1, p2, ns, ntab, nfft, pairs, amp=None):
    import torch

    from pyimcom_amd._lib import check, lib

    ctx = _ctx()
    dev = torch.device("cuda:0")
    t1, t2 = torch.as_tensor(np.ascontiguousarray(p1), device=dev), torch.as_tensor(np.ascontiguousarray(p2), device=dev)
    pairs = np.array(pairs, dtype=np.int32)
    out = torch.full((len(pairs), ntab + 12, ntab + 12), np.nan, dtype=torch.float64, device=dev)
    check(lib.imcom_psf_overlap_wide(ctx.handle, _dp(t1), t1.shape[0], _dp(t2), t2.shape[0], ns, ntab, nfft, _hp(pairs), len(pairs),
                                     None if amp is None else _hp(amp), _dp(out)))
    o = out.cpu().numpy()
    border = o.copy()
    border[:, 6:-6, 6:-6] = 0.0
    assert np.all(border == 0.0)  # every border element written, none left at the NaN fill
    return o[:, 6:-6, 6:-6]


def _spectra(p, ns, nfft):
    import torch

    from pyimcom_amd._lib import check, lib

    ctx = _ctx()
    t = torch.as_tensor(np.ascontiguousarray(p), device="cuda:0")
    size = int(lib.imcom_psf_spectra_size(ns, nfft))
    assert size > 0
    spec = torch.empty((t.shape[0], size), dtype=torch.float64, device="cuda:0")
    check(lib.imcom_psf_spectra(ctx.handle, _dp(t), t.shape[0], ns, nfft, _dp(spec)))
    return spec


def _wide_from_spectra(s1, s2, ns, ntab, nfft, pairs, amp=None, win=None, slots=None, out=None):
    import torch

    from pyimcom_amd._lib import check, lib

    ctx = _ctx()
    pairs = np.array(pairs, dtype=np.int32)
    if out is None:
        out = torch.full((len(pairs), ntab + 12, ntab + 12), np.nan, dtype=torch.float64, device="cuda:0")
    check(lib.imcom_psf_overlap_spectra_wide(ctx.handle, _dp(s1), s1.shape[0], _dp(s2), s2.shape[0], ns, ntab, nfft, _hp(pairs), len(pairs),
                                             None if amp is None else _hp(amp), None if win is None else _hp(win), None if slots is None else _hp(slots),
                                             out.shape[0], _dp(out)))
    return out


def _rel(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


SELF = [(i, j) for i in range(3) for j in range(i, 3)]


@pytest.mark.parametrize("tag", ["a", "b"])
@pytest.mark.parametrize("route", ["plan", "gemm"])
def test_wide_tables_from_psfs_golden(golden, tag, route, monkeypatch):
    """imcom_psf_overlap_wide against PSFOvl's tables under psfsplit, both geometries of the fixture (nfft 64 = 16 4 and 60 = 4 3 5), on
    the butterfly route and on the dense-DFT route (IMCOM_PSF_OVERLAP=gemm, the route of sizes without a plan)."""
    if route == "gemm":
        monkeypatch.setenv("IMCOM_PSF_OVERLAP", "gemm")
    g = golden("psfsplit")
    _, ns, nfft, ntab = _sizes(g, tag)
    p1, p2, po = g[f"{tag}_psf1"], g[f"{tag}_psf2"], g[f"{tag}_psfo"]
    tri = _wide_from_psfs(p1, p1, ns, ntab, nfft, SELF)
    ref = g["a_ovl_self"] if tag == "a" else g["b_ovl_self_0"]
    print("self", tag, route, _rel(tri[: len(ref)], ref))
    assert _rel(tri[: len(ref)], ref) < TAB
    io = _wide_from_psfs(p1, po, ns, ntab, nfft, [(i, 0) for i in range(3)])
    print("io", _rel(io, g[f"{tag}_ovl_io"][:, 0]))
    assert _rel(io, g[f"{tag}_ovl_io"][:, 0]) < TAB
    cc = _wide_from_psfs(po, po, ns, ntab, nfft, [(0, 0)])
    assert abs(cc[0, ntab // 2, ntab // 2] - g[f"{tag}_outovlc"][0]) < 1e-13 * g[f"{tag}_outovlc"][0]
    if tag == "a":
        cross = _wide_from_psfs(p1, p2, ns, ntab, nfft, [(i, j) for i in (0, 2) for j in range(3)]).reshape(2, 3, ntab, ntab)
        print("cross", _rel(cross, g["a_ovl_cross_02"]))
        assert _rel(cross, g["a_ovl_cross_02"]) < TAB


@pytest.mark.parametrize("tag", ["a", "b"])
def test_wide_tables_from_spectra_windows_slots_and_narrow_centre(golden, tag):
    """imcom_psf_overlap_spectra_wide on the fixture: whole tables against the reference; windowed tables equal the whole ones on their
    windows bit for bit; tables written into the slots of an arena; and the central nsamp x nsamp window of a wide table against the narrow
    entry (imcom_psf_overlap_spectra) on the same spectra -- the reference has the two equal bit for bit, the device runs the kept rows
    through different launches."""
    import torch

    from pyimcom_amd._lib import ImcomError, check, lib

    g = golden("psfsplit")
    _, ns, nfft, ntab = _sizes(g, tag)
    spec = _spectra(np.concatenate([g[f"{tag}_psf1"], g[f"{tag}_psfo"]]), ns, nfft)
    pairs = SELF + [(i, 3) for i in range(3)]
    full = _wide_from_spectra(spec, spec, ns, ntab, nfft, pairs)
    f = full.cpu().numpy()
    ref = np.concatenate([g["a_ovl_self"] if tag == "a" else g["b_ovl_self_0"]])
    assert _rel(f[: len(ref), 6:-6, 6:-6], ref) < TAB and _rel(f[6:, 6:-6, 6:-6], g[f"{tag}_ovl_io"][:, 0]) < TAB
    border = f.copy()
    border[:, 6:-6, 6:-6] = 0.0
    assert np.all(border == 0.0)
    # windows (table coordinates 0..ntab)
    nc = ntab // 2
    win = np.array([[0, nc + 8, 0, ntab], [nc - 8, ntab, nc - 8, ntab], [3, nc, 0, nc + 8], [0, ntab, 0, ntab], [nc - 10, nc + 11, nc - 10, nc + 11]] * 2,
                   dtype=np.int32)[: len(pairs)]
    part = _wide_from_spectra(spec, spec, ns, ntab, nfft, pairs, win=win).cpu().numpy()
    for q, (r0, r1, c0, c1) in enumerate(win):
        assert np.array_equal(part[q, 6 + r0 : 6 + r1, 6 + c0 : 6 + c1], f[q, 6 + r0 : 6 + r1, 6 + c0 : 6 + c1]), q
    bad = win.copy()
    bad[0, 1] = ntab + 1
    with pytest.raises(ImcomError):
        _wide_from_spectra(spec, spec, ns, ntab, nfft, pairs, win=bad)
    # slots of an arena
    arena = torch.zeros((12, ntab + 12, ntab + 12), dtype=torch.float64, device="cuda:0")
    slots = np.array([7, 2, 9, 4, 11, 0, 5, 1, 3], dtype=np.int32)
    _wide_from_spectra(spec, spec, ns, ntab, nfft, pairs, slots=slots, out=arena)
    a = arena.cpu().numpy()
    assert np.array_equal(a[slots], f) and not a[[6, 8, 10]].any()
    # the centre of the wide table against the narrow entry on the same spectra
    pr = np.array(pairs, dtype=np.int32)
    narrow = torch.empty((len(pairs), ns + 12, ns + 12), dtype=torch.float64, device="cuda:0")
    check(lib.imcom_psf_overlap_spectra(_ctx().handle, _dp(spec), 4, _dp(spec), 4, ns, nfft, _hp(pr), len(pr), None, _dp(narrow)))
    n = narrow.cpu().numpy()[:, 6:-6, 6:-6]
    lo = 6 + nc - ns // 2
    print("centre vs narrow", tag, _rel(f[:, lo : lo + ns, lo : lo + ns], n))
    assert _rel(f[:, lo : lo + ns, lo : lo + ns], n) < TAB
    # a table side that is not a table side is refused
    for bad_ntab in (ntab + 1, ntab + 2, ns - 2):
        with pytest.raises(ImcomError):
            _wide_from_spectra(spec, spec, ns, bad_ntab, nfft, pairs)


def test_wide_tables_amp_penalty_golden(golden):
    """cfg.amp_penalty (psfutil.py:661-671) through PSFGroupTables with a table side of its own, against the reference's wide table and C;
    and without the weighting (amp_penalty off) against the restatement."""
    from pyimcom_amd import psfs
    from pyimcom_amd.stamps import PSFGroupTables
    from tests import psfsplit_reference as psr

    g = golden("psfsplit")
    ov, ns, nfft, ntab = _sizes(g, "a")
    a0, a1 = g["amp_penalty"]
    s0, s1 = (float(v) for v in g["amp_targets"])
    mk = lambda kind, sig: psfs.sample_psf(psfs.get_outpsf(kind, sig, 2, ns, ov)[None], ns, None, True, True)  # noqa: E731
    tabs = PSFGroupTables(mk("GAUSSIAN", s0), mk("AIRYOBSC", s1), nfft, amp_penalty=(a0, a1 * ov), ntab=ntab)
    assert tuple(tabs.tables.shape[1:]) == (ntab + 12, ntab + 12)
    got = tabs.tables[tabs.ntri].cpu().numpy()[6:-6, 6:-6]
    ref = g["amp_ovl_io"][0, 0]
    print("amp", _rel(got, ref), abs(tabs.C - g["amp_outovlc"][0]) / tabs.C)
    assert np.abs(got - ref).max() <= 5e-13 * np.abs(ref).max()
    assert abs(tabs.C - g["amp_outovlc"][0]) <= 1e-12 * tabs.C
    plain = PSFGroupTables(mk("GAUSSIAN", s0), mk("AIRYOBSC", s1), nfft, ntab=ntab)
    sg = psr.SplitGeom(int(g["a_pars"][0]), ov, 0.04 / 3600.0, 0.0)
    rt, rC = psr.table_set(mk("GAUSSIAN", s0), mk("AIRYOBSC", s1), sg)
    assert np.abs(plain.tables.cpu().numpy()[:, 6:-6, 6:-6] - rt).max() <= 5e-13 * np.abs(rt).max() and abs(plain.C - rC[0]) <= 1e-12 * plain.C
    assert abs(plain.C - tabs.C) > 0.05 * tabs.C  # the weighting really changes the numbers


def test_wide_tables_production_size():
    """One table set at production size (npixpsf 48, oversamp 8: PSF side 383, nfft 768 = 16 16 3, table side 767; the static kernels)
    against numpy's FFTs, whole and windowed: a windowed call equals the whole table on its window bit for bit and -- as for the unsplit
    tables -- writes nothing else but zero-border cells (the row transform works on row pairs)."""
    ns, nfft, ntab = 383, 768, 767
    rng = np.random.default_rng(ns)
    yy, xx = np.mgrid[:ns, :ns] - ns // 2
    p = np.stack([np.exp(-(xx**2 + yy**2) / (2.0 * (6.0 + 1.5 * k) ** 2)) + 1e-3 * rng.standard_normal((ns, ns)) for k in range(3)])
    p /= p.sum(axis=(1, 2))[:, None, None]
    fpad = np.zeros((3, nfft, nfft))
    fpad[:, :ns, :ns] = p
    r = np.fft.rfft2(fpad)
    pairs = [(0, 1), (1, 2), (2, 0), (1, 1)]
    nc = ntab // 2
    ref = np.stack([np.roll(np.fft.irfft2(r[i] * np.conj(r[j]), s=(nfft, nfft)), (nc, nc), axis=(0, 1))[:ntab, :ntab] for i, j in pairs])
    spec = _spectra(p, ns, nfft)
    f = _wide_from_spectra(spec, spec, ns, ntab, nfft, pairs).cpu().numpy()
    print("production whole", _rel(f[:, 6:-6, 6:-6], ref))
    assert _rel(f[:, 6:-6, 6:-6], ref) < TAB
    border = f.copy()
    border[:, 6:-6, 6:-6] = 0.0
    assert np.all(border == 0.0)
    win = np.array([[0, nc + 8, 0, ntab], [nc - 8, ntab, nc - 8, ntab], [nc - 60, nc + 61, nc - 90, nc + 91], [3, nc, 0, nc + 8]], dtype=np.int32)
    import torch

    part = torch.full((4, ntab + 12, ntab + 12), -7.0, dtype=torch.float64, device="cuda:0")
    g = _wide_from_spectra(spec, spec, ns, ntab, nfft, pairs, win=win, out=part).cpu().numpy()
    for q, (r0, r1, c0, c1) in enumerate(win):
        assert np.array_equal(g[q, 6 + r0 : 6 + r1, 6 + c0 : 6 + c1], f[q, 6 + r0 : 6 + r1, 6 + c0 : 6 + c1]), q
        inside = np.zeros(g[q].shape, bool)
        lo, hi = 2 * (r0 // 2), min(2 * ((r1 + 1) // 2), ntab)
        inside[6 + lo : 6 + hi, 6 + c0 : 6 + c1] = True
        untouched = g[q] == -7.0
        assert np.all(untouched[~inside & (f[q] != 0.0)]), q
        assert not untouched[inside].any(), q
    # the dense-DFT route at this size through the same entry point is exercised on the fixture's sizes; here: from PSFs, butterfly route
    d = _wide_from_psfs(p, p, ns, ntab, nfft, pairs)
    assert np.array_equal(d, f[:, 6:-6, 6:-6])  # spectra + inverse in one call: the same launches


def test_affine_positions_and_sampling_golden(golden):
    """imcom_affine_positions against the positions the reference formed from four evaluations of a NON-affine pixel map (psfutil.py:
    739-753), host and device memory, and ``sample_psf`` on them against the reference's sampled PSFs.  The device forms the same two
    products and one sum per element from the same operands: the bound is 4 ulp of the largest coordinate (the test prints the observed distance)."""
    import torch

    from pyimcom_amd import psfs

    g = golden("psfsplit")
    _, ns, _, _ = _sizes(g, "a")
    card, ref = g["samp_cardinal"], g["samp_yxco"]
    got_h = psfs.affine_positions(card, ns)
    got_d = psfs.affine_positions(torch.as_tensor(card, device="cuda:0"), ns)
    assert np.array_equal(got_h, got_d.cpu().numpy())
    err = float(np.abs(got_h - ref).max())
    print("affine positions: max |d| =", err, "of", float(np.abs(ref).max()))
    assert err <= 4 * np.spacing(np.abs(ref).max())
    arr = psfs.sample_psf(torch.as_tensor(g["samp_psf"], device="cuda:0"), ns, got_d).cpu().numpy()
    assert np.abs(arr - g["samp_psf_arr"]).max() <= 1e-13 * np.abs(g["samp_psf_arr"]).max()


def test_builders_on_wide_tables_golden(golden):
    """imcom_build_A / imcom_build_B on wide tables against PSFOvl.__call__ of the reference for InStamps whose separations lie off the
    unsplit table: one PSF group (self sub-blocks, input-output sub-block) through PSFGroupTables, two groups (cross sub-block) through
    BlockTables -- both with the table side 2 nsamp + 1."""
    import torch

    from pyimcom_amd._lib import TableGeom, check, lib
    from pyimcom_amd.stamps import BlockTables, PSFGroupTables
    from tests.parity import TOL

    g = golden("psfsplit")
    _, ns, nfft, ntab = _sizes(g, "a")
    fp, dscale = 1e-7, float(g["a_dscale"])
    dev = torch.device("cuda:0")
    geom = TableGeom(ntab, float(ntab // 2), dscale, fp)
    c1, c2 = g["st1_count"].astype(int), g["st2_count"].astype(int)
    x = np.concatenate([g["st1_x"], g["st2_x"]])
    y = np.concatenate([g["st1_y"], g["st2_y"]])
    e1, e2 = np.repeat(np.arange(3), c1), np.repeat(np.arange(3), c2)
    n, ldn, ldm, n2f = x.size, 128, 128, 6

    def pad(a, dt):
        out = np.zeros((1, ldn), dt)
        out[0, : a.size] = a
        return torch.as_tensor(out, device=dev)

    xd, yd = pad(x, np.float64), pad(y, np.float64)
    nn = np.array([n], dtype=np.int32)

    def build_A(tables, psf, tab, pen):
        P = tab.shape[-1]
        A = torch.empty((1, ldn, ldn), dtype=torch.float64, device=dev)
        tt, pp = torch.as_tensor(tab.reshape(1, P, P).astype(np.int32), device=dev), torch.as_tensor(pen.reshape(1, P, P).astype(np.float64), device=dev)
        check(lib.imcom_build_A(_ctx().handle, 1, _hp(nn), ldn, _dp(xd), _dp(yd), _dp(psf), _dp(tables), tables.shape[0], C.byref(geom), _dp(tt), _dp(pp), P, _dp(A)))
        return A.cpu().numpy()[0, :n, :n]

    # one group: both InStamps' pixels carry PSFs of group 1
    one = PSFGroupTables(g["a_psf1"], g["a_psfo"], nfft, ntab=ntab)
    assert one.ntab == ntab and abs(one.C - g["a_outovlc"][0]) <= 1e-12 * one.C
    tab, pen, io = one.pair_maps(fp)
    A = build_A(one.tables, pad(np.concatenate([e1, e2]), np.int32), tab, pen)
    scale = np.abs(g["A_self_11"]).max()
    e11, e12 = np.abs(A[:9, :9] - g["A_self_11"]).max() / scale, np.abs(A[:9, 9:] - g["A_self_12"]).max() / scale
    print("A self", e11, e12)
    assert e11 < TOL["A"] and e12 < TOL["A"]
    Bt = torch.empty((1, ldn, ldm), dtype=torch.float64, device=dev)
    iod = torch.as_tensor(io.reshape(1, -1).astype(np.int32), device=dev)
    ox0, oy0 = torch.tensor([float(g["out_yx"][1, 0, 0])], dtype=torch.float64, device=dev), torch.tensor([float(g["out_yx"][0, 0, 0])], dtype=torch.float64, device=dev)
    n1 = np.array([9], dtype=np.int32)
    check(lib.imcom_build_B(_ctx().handle, 1, _hp(n1), ldn, _dp(xd), _dp(yd), _dp(pad(e1, np.int32)), _dp(one.tables), one.tables.shape[0], C.byref(geom),
                            _dp(iod), one.n_psf, _dp(ox0), _dp(oy0), n2f, ldm, _dp(Bt)))
    B = Bt.cpu().numpy()[0, :9, : n2f * n2f].T
    eB = np.abs(B - g["B_io_1all"][0]).max() / np.abs(g["B_io_1all"]).max()
    print("B io", eB)
    assert eB < TOL["B"]
    sel = g["sel1"].astype(int)
    assert np.abs(B[:, sel] - g["B_io_1sel"][0]).max() / np.abs(g["B_io_1all"]).max() < TOL["B"]
    # two groups: the second InStamp's pixels carry PSFs of group 2 -> the cross sub-block
    bt = BlockTables({(0, 0): g["a_psf1"], (0, 1): g["a_psf2"]}, g["a_psfo"], nfft, ntab=ntab)
    groups = [(0, 0), (0, 1)]
    bt.require(BlockTables.keys_for(groups))
    tab, pen, io, lut = bt.stamp_maps(groups, fp)
    slot = np.concatenate([lut[0, e1], lut[1, e2]])
    A2 = build_A(bt.tables, pad(slot, np.int32), tab, pen)
    ex = np.abs(A2[:9, 9:] - g["A_cross_12"]).max() / scale
    print("A cross", ex)
    assert ex < TOL["A"] and np.abs(A2[:9, :9] - g["A_self_11"]).max() / scale < TOL["A"]


def _split_block(golden, kernel, kC):
    from tests.test_gpu_refblock import reference_block

    g = golden("stamp_chain")
    blk, psfgrp = reference_block(g, kernel, kC)
    blk.cfg.psfsplit = [3.0, 6.0, 1e-3]  # PSFSPLIT = (r1, r2, epsilon) of the configuration: the seam only asks whether it is set
    return g, blk, psfgrp


@pytest.mark.parametrize("kernel,kC", [("Cholesky", [2e-3]), ("Eigen", [1e-4, 1e-1])])
def test_block_seam_psfsplit_whole_block_vs_restatement(golden, kernel, kC):
    """``coadd_output_stamps(..., psfsplit=True)`` on the duck-typed block of tests/golden/stamp_chain.npz (affine pixel maps) against the
    restatement's stamp loop with wide tables and four-point positions, every block array, at the bounds of
    tests/test_gpu_refblock.py::test_block_seam_whole_block_vs_oracle; without the keyword the same block is refused; a PSFGrp that says
    otherwise is an error."""
    from pyimcom_amd._lib import ImcomError
    from pyimcom_amd.blockrun import stamp_neighbours
    from pyimcom_amd.refblock import IMCOM_ERR_UNSUPPORTED, coadd_output_stamps
    from tests import psfsplit_reference as psr

    g, blk, psfgrp = _split_block(golden, kernel, kC)
    fp = float(g["flat_penalty"])
    with pytest.raises(ImcomError) as ei:
        coadd_output_stamps(blk, psfgrp, flat_penalty=fp, batch=3)
    assert ei.value.status == IMCOM_ERR_UNSUPPORTED and not hasattr(blk, "out_map")
    psfgrp.psfsplit = False
    with pytest.raises(ValueError):
        coadd_output_stamps(blk, psfgrp, flat_penalty=fp, batch=3, psfsplit=True)
    psfgrp.psfsplit = True
    maps = coadd_output_stamps(blk, psfgrp, flat_penalty=fp, batch=3, psfsplit=True)
    ref = psr.block_loop(g, kernel, kC, fp, stamp_neighbours)
    assert blk.out_map.shape == (1, blk.cfg.n_inframe, maps.nside, maps.nside)
    a, b = blk.out_map, ref["out_map"]
    assert np.isfinite(a).all() and np.abs(b).max() > 0
    print("out_map", np.abs(a - b).max() / np.abs(b).max())
    assert np.abs(a - b).max() <= 5e-5 * np.abs(b).max(), np.abs(a - b).max() / np.abs(b).max()
    for k in ("UC_map", "Sigma_map", "kappa_map", "Tsum_map", "Neff_map", "T_weightmap"):
        a, b = getattr(blk, k), ref[k]
        assert a.shape == b.shape and np.allclose(a, b, rtol=5e-5, atol=2e-6 * np.abs(b).max()), (k, np.abs(a - b).max(), np.abs(b).max())


def test_block_seam_psfsplit_does_not_depend_on_the_table_cache():
    """The maps of a PSFSPLIT block do not depend on how many wide tables stay resident: an arena that holds the sets of one cell of 2 x 2
    stamps (every pass evicts) against one that holds the whole block -- bit for bit, as for the unsplit tables."""
    import dataclasses

    from pyimcom_amd import synth
    from pyimcom_amd.blockrun import tile_tables
    from pyimcom_amd.refblock import coadd_output_stamps

    n1P, E = 6, 3
    wl = dataclasses.replace(synth.CONFIGS["small"], n_expo=E)
    outs = []
    for cap in (None, tile_tables(1, 1, E, 1)):
        blk, psfgrp, _, _ = synth.duck_block(wl, n1P, E, seed=8)
        blk.cfg.psfsplit = [3.0, 6.0, 1e-3]
        coadd_output_stamps(blk, psfgrp, flat_penalty=wl.flat_penalty, batch=4, table_capacity=cap, psfsplit=True)
        outs.append({k: getattr(blk, k).copy() for k in ("out_map", "UC_map", "Sigma_map", "kappa_map", "Tsum_map", "Neff_map", "T_weightmap")})
    assert np.abs(outs[0]["out_map"]).max() > 0
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k
