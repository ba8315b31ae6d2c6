"""The coaddition epilogue (OutStamp._perform_coaddition, coadd.py:1320-1354) on the device, directly through the C-ABI, at its lane,
frame, row and exposure edges: imcom_coadd_epilogue (coadd_epilogue_kernel<4> / <1>, tsum_stamp_kernel) on every case of
tests/epilogue_reference.py CASES with everything the kernel must not use poisoned, ragged batches against their stamps run alone,
the map taper imcom_trapezoid_f32, and the coaddition inside imcom_solve_chol_resident_coadd (tile_coadd_partials,
coadd_from_partials_kernel) on FUSED_CASES, judged on the T the call returned.  Reference, bounds and comparator: epilogue_reference
(its CPU pin is tests/test_epilogue_reference.py)."""

import ctypes as C

import numpy as np
import pytest

from tests import epilogue_reference as ep

pytestmark = pytest.mark.gpu

SENT = 7.0  # outputs are pre-filled with this: everything must be overwritten
OUTS = ("outimage", "Tsum_stamp", "Tsum_inpix", "Neff")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(t):
    """A float tensor as integers: equality of bits (a NaN equals itself)."""
    import torch

    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same(a, b):
    import torch

    return torch.equal(_bits(a), _bits(b))


def _outputs(batch, n_inframe, n_expo, m, dev):
    import torch

    return dict(outimage=torch.full((batch, n_inframe, m), SENT, dtype=torch.float32, device=dev),
                Tsum_stamp=torch.full((batch, n_expo), SENT, dtype=torch.float64, device=dev),
                Tsum_inpix=torch.full((batch, m), SENT, dtype=torch.float64, device=dev),
                Neff=torch.full((batch, m), SENT, dtype=torch.float64, device=dev))


def _poisoned(case, data, stamps):
    """Copies of the stamps' Tt / indata / expo with what the kernel must not use made poisonous: rows >= n and columns >= m of Tt and
    the tail of indata NaN, the tail of expo 2^30."""
    Tt, x, e = (np.array(a[stamps]) for a in data)
    for k, s in enumerate(stamps):
        ns = case.ns[s]
        Tt[k, ns:, :] = np.nan
        Tt[k, :, case.m:] = np.nan
        x[k, :, ns:] = np.nan
        e[k, ns:] = 2**30
    return Tt, x, e


def _epilogue(case, data, stamps=None):
    """imcom_coadd_epilogue on the stamps `stamps` of the case (None: all of them).  Returns the outputs and Tt as device tensors."""
    import torch

    from pyimcom_amd._dev import bound_context
    from pyimcom_amd._lib import check, lib, ptr

    stamps = list(range(len(case.ns))) if stamps is None else list(stamps)
    dev = torch.device("cuda:0")
    Tt, x, e = (torch.from_numpy(a).to(dev) for a in _poisoned(case, data, stamps))
    ns = np.array([case.ns[s] for s in stamps], np.int32)
    out = _outputs(len(stamps), case.n_inframe, case.n_expo, case.m, dev)
    ctx = bound_context(dev)
    check(lib.imcom_coadd_epilogue(ctx.handle, len(stamps), _p(ns), case.ldn, case.m, case.ldm, case.n2f, case.fade, case.n2, ptr(Tt), ptr(x),
                                   case.n_inframe, ptr(e), case.n_expo, ptr(out["outimage"]), ptr(out["Tsum_stamp"]), ptr(out["Tsum_inpix"]),
                                   ptr(out["Neff"])))
    torch.cuda.synchronize()
    out["T"] = Tt
    return out


def _numpy(out):
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ the stand-alone epilogue
@pytest.mark.parametrize("case", ep.CASES, ids=lambda c: c.name)
def test_stand_alone_epilogue(case):
    """Every case against the long-double reference within the derived bounds (the exact family: bit for bit), the poison nowhere in
    the outputs, the returned T equal to the reference's tapered T in the rows < n and columns < m."""
    data = case.inputs()
    got = _numpy(_epilogue(case, data))
    ref = case.reference(data)
    for k in ("outimage", "Tsum_stamp", "Tsum_inpix"):
        assert np.isfinite(got[k]).all(), k
    worst = ep.compare(got, ref, case)
    print(f"[epilogue edges] {case.name}: {ep.fmt(worst)}")
    assert max(worst.values()) <= 1.0, (case.name, ep.fmt(worst))


@pytest.mark.parametrize("case", ep.CASES, ids=lambda c: c.name)
def test_ragged_batch_equals_its_stamps_alone(case):
    """Each stamp of the batch run alone gives the bits it gives in the batch; the same call twice gives the same bits."""
    data = case.inputs()
    a, b = _epilogue(case, data), _epilogue(case, data)
    for k in OUTS:
        assert _same(a[k], b[k]), (case.name, k)
    for s, ns in enumerate(case.ns):
        assert _same(a["T"][s, :ns, : case.m], b["T"][s, :ns, : case.m])
        one = _epilogue(case, data, [s])
        for k in OUTS:
            assert _same(one[k][0], a[k][s]), (case.name, s, k)
        assert _same(one["T"][0, :ns, : case.m], a["T"][s, :ns, : case.m]), (case.name, s)


@pytest.mark.parametrize("n2,fade", ep.FADES)
def test_map_taper(n2, fade):
    """imcom_trapezoid_f32 on three random float32 maps equals oracle.trapezoid bit for bit, overlapping ramps included."""
    import torch

    from oracle import oracle as orc
    from pyimcom_amd._dev import bound_context
    from pyimcom_amd._lib import check, lib, ptr

    n2f = n2 + 2 * fade
    maps = np.random.default_rng(n2f).standard_normal((3, n2f, n2f)).astype(np.float32)
    dev = torch.device("cuda:0")
    t = torch.from_numpy(maps).to(dev)
    check(lib.imcom_trapezoid_f32(bound_context(dev).handle, ptr(t), 3, n2f, fade))
    torch.cuda.synchronize()
    want = maps.copy()
    orc.trapezoid(want, fade)
    assert not np.array_equal(want, maps) and np.array_equal(t.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ the coaddition inside the solve
def _fused(case, fade=0):
    """imcom_solve_chol_resident_coadd on the case; the tails of indata and expo poisoned.  Returns the outputs, Tt (device tensors),
    info and the unpoisoned host indata / expo / -B/2."""
    import torch

    from pyimcom_amd._dev import bound_context
    from pyimcom_amd._lib import check, lib, ptr

    A, Bt, Cs, x, e = case.inputs()
    xp, epz = x.copy(), e.copy()
    for s, ns in enumerate(case.ns):
        xp[s, :, ns:] = np.nan
        epz[s, ns:] = 2**30
    dev = torch.device("cuda:0")
    batch, m, ldn, ldm = len(case.ns), case.m, case.ldn, case.ldm
    A_d, Bt_d, x_d, e_d = (torch.from_numpy(a).to(dev) for a in (A, Bt, xp, epz))
    Tt = torch.zeros((batch, ldn, ldm), dtype=torch.float32, device=dev)
    UC, Sg, kp = (torch.full((batch, m), SENT, dtype=torch.float32, device=dev) for _ in range(3))
    out = _outputs(batch, case.n_inframe, case.n_expo, m, dev)
    ns = np.array(case.ns, np.int32)
    kC = np.array(case.kappaC, np.float64)
    info = np.full(batch, -7, np.int32)
    ctx = bound_context(dev)
    check(lib.imcom_solve_chol_resident_coadd(ctx.handle, batch, _p(ns), ldn, m, ldm, ptr(A_d), ptr(Bt_d), _p(Cs), _p(kC), kC.size, 1e-4, 1.0,
                                              ptr(Tt), ptr(UC), ptr(Sg), ptr(kp), _p(info), case.n2f, fade, case.n2, ptr(x_d), case.n_inframe,
                                              ptr(e_d), case.n_expo, ptr(out["outimage"]), ptr(out["Tsum_stamp"]), ptr(out["Tsum_inpix"]),
                                              ptr(out["Neff"])))
    torch.cuda.synchronize()
    assert np.array_equal(A_d.cpu().numpy(), A) and np.array_equal(Bt_d.cpu().numpy(), Bt)  # the inputs are not modified
    out["T"] = Tt
    return out, info, (x, e, Bt)


def _judge_fused(case, out, host):
    """The coaddition against the reference evaluated on the T the call returned (float32: exact input -- the coaddition is judged,
    not the solve); the cap on S / sabs that the real family's bounds assume, on that T."""
    x, e, _ = host
    got = _numpy(out)
    Tt = got["T"]
    for s, ns in enumerate(case.ns):
        assert np.isfinite(Tt[s, :ns]).all() and np.all(Tt[s, :ns, case.m:] == 0), (case.name, s)
    ref = ep.reference(Tt, x, e, case.ns, case.n_expo, case.n2f, case.n2, 0)
    if not case.exact:
        for s, ns in enumerate(case.ns):
            assert ns == 0 or float((ref["S"][s] / ref["sabs"][s]).max()) <= ep.CAP, (case.name, s)
    got["T"] = None
    worst = ep.compare(got, ref, case)
    print(f"[epilogue edges] {case.name}: {ep.fmt(worst)}")
    assert max(worst.values()) <= 1.0, (case.name, ep.fmt(worst))


@pytest.mark.parametrize("case", [c for c in ep.FUSED_CASES if c.kind == "plain"], ids=lambda c: c.name)
def test_coaddition_inside_the_solve(case):
    """Ragged batches n = 0, 1, 127, 128, 129, 300 (one to three block rows, the last one ragged), odd and even exposure counts, m on
    one and on three column tiles."""
    out, info, host = _fused(case)
    assert info.tolist() == [0] * len(case.ns)
    _judge_fused(case, out, host)


def test_coaddition_inside_the_solve_identity_batch():
    """A + kappa I == I and -B/2 of the exact family: the solve multiplies by 0 and 1, T is float32(-B/2), and the coaddition is held
    bit for bit like the stand-alone exact family."""
    case = next(c for c in ep.FUSED_CASES if c.kind == "identity")
    out, info, host = _fused(case)
    assert info.tolist() == [0] * len(case.ns)
    Tt = out["T"].cpu().numpy()
    for s, ns in enumerate(case.ns):
        assert np.array_equal(Tt[s, :ns], host[2][s, :ns].astype(np.float32)), s
    _judge_fused(case, out, host)


def test_coaddition_inside_the_solve_survives_a_repair():
    """One stamp's first factorisation fails and a later attempt repairs and solves it alone (lakernel.py:262-279): its sums match its
    own T, and the other stamps' pieces, written by the first attempt, are what they are in the same batch without the failure.  With
    two kappa nodes the stand-alone epilogue runs inside the call: the same bounds against the returned T."""
    cases = {c.name: c for c in ep.FUSED_CASES}
    case = cases["fused-repair"]
    out, info, host = _fused(case)
    assert info[ep.REPAIR_AT] != 0 and not np.delete(info, ep.REPAIR_AT).any(), info
    _judge_fused(case, out, host)
    ctl, info_c, host_c = _fused(ep.REPAIR_CONTROL)
    assert not info_c.any()
    _judge_fused(ep.REPAIR_CONTROL, ctl, host_c)
    keep = [s for s in range(len(case.ns)) if s != ep.REPAIR_AT]
    for k in OUTS + ("T",):
        assert _same(out[k][keep], ctl[k][keep]), k
    assert not _same(out["T"][ep.REPAIR_AT], ctl["T"][ep.REPAIR_AT])
    two, info_2, host_2 = _fused(ep.REPAIR_TWO_NODES)
    assert info_2[ep.REPAIR_AT] != 0 and not np.delete(info_2, ep.REPAIR_AT).any(), info_2
    _judge_fused(ep.REPAIR_TWO_NODES, two, host_2)


# ------------------------------------------------------------------------------------------------ what the entries refuse
def test_refusals():
    """Host checks, before anything is launched: more than 64 exposures, a fade in the fused entry, an ldm that is no multiple of 128,
    an ldn below a stamp's n.  The outputs keep their fill."""
    import torch

    from pyimcom_amd._dev import bound_context
    from pyimcom_amd._lib import ImcomError, check, lib, ptr

    dev = torch.device("cuda:0")
    ctx = bound_context(dev)
    n2f, m, ldn, ldm, nf = 3, 9, 256, 128, 1
    ns = np.array([33], np.int32)

    def call(n_expo=3, ldn_arg=ldn, ldm_arg=ldm):
        Tt = torch.zeros((1, ldn, ldm), dtype=torch.float32, device=dev)  # (full size whatever the arguments say)
        x = torch.zeros((1, nf, ldn), dtype=torch.float32, device=dev)
        e = torch.zeros((1, ldn), dtype=torch.int32, device=dev)
        out = _outputs(1, nf, n_expo, m, dev)
        rc = lib.imcom_coadd_epilogue(ctx.handle, 1, _p(ns), ldn_arg, m, ldm_arg, n2f, 0, n2f, ptr(Tt), ptr(x), nf, ptr(e), n_expo,
                                      ptr(out["outimage"]), ptr(out["Tsum_stamp"]), ptr(out["Tsum_inpix"]), ptr(out["Neff"]))
        torch.cuda.synchronize()
        for k in OUTS:  # a refused call has written nothing, an accepted one everything
            assert bool((out[k] == SENT).all()) == (rc != 0) and bool((out[k] == SENT).any()) == (rc != 0), k
        check(rc)

    with pytest.raises(ImcomError, match="n_expo"):
        call(n_expo=65)
    with pytest.raises(ImcomError, match="ldm=9 must be a multiple of 128"):
        call(ldm_arg=9)
    with pytest.raises(ImcomError, match="ldm=132 must be a multiple of 128"):
        call(ldm_arg=132)
    with pytest.raises(ImcomError, match="ldn=32 is below"):
        call(ldn_arg=32)
    call()  # (the same call with the layout every caller passes goes through)
    case = next(c for c in ep.FUSED_CASES if c.kind == "plain" and c.m == 9)
    with pytest.raises(ImcomError, match="fade"):
        _fused(case, fade=1)
