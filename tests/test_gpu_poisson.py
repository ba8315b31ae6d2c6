"""numpy's Poisson draws and the nstar layer on the device (csrc/poisson.hip, pyimcom_amd.noiselayers.poisson, pyimcom_amd.inject.nstar_layer):
every comparison is bit-for-bit equality with numpy's own generator, computed here.  The seeds the cases are built around are searched on
the CPU with the Python restatement (tests/poisson_reference.py).

Tiles and superchunks are runs of DRAWS here (a draw's position depends on the draws before it), so "an event at the first / last position
of a tile" is an event in the first / last draw of a tile."""

import os

import numpy as np
import pytest

from tests import poisson_reference as pr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [dict(_superchunk=16, _tile=4, _window=64), dict(_superchunk=256, _tile=64)]


def _numpy(seed, lam, offset=0):
    bg = np.random.PCG64(seed)
    if offset:
        bg.advance(offset)
    return np.random.Generator(bg).poisson(lam=lam), bg


def _check(seed, lam, offset=0, **kw):
    from pyimcom_amd import noiselayers as nl

    lam = np.asarray(lam, dtype=np.float64)
    want, left = _numpy(seed, lam, offset)
    bg = np.random.PCG64(seed)
    got, info = nl.poisson(bg, lam, offset=offset, return_info=True, **kw)
    assert got.shape == want.shape and got.dtype == np.int64
    assert got.tobytes() == want.tobytes(), (np.flatnonzero(got.ravel() != want.ravel())[:5], info)
    assert bg.state == left.state
    return got, info


def _rates(n):
    """Mostly the background, with rates below 10 and zeros sprinkled in."""
    lam = np.full(n, 86.0)
    lam[3::7] = 3.0
    lam[5::11] = 0.0
    return lam


@pytest.mark.parametrize("geom", GEOMETRIES, ids=["S16_T4", "S256_T64"])
@pytest.mark.parametrize("count", ["0", "1", "T-1", "T", "T+1", "S-1", "S", "S+1", "3*S+5"])
def test_counts_around_tile_and_superchunk(geom, count):
    n = eval(count, {"T": geom["_tile"], "S": geom["_superchunk"]})
    _, info = _check(4242, _rates(n), **geom)
    assert info["undecided"] == 0 and info["consumed"] >= n


@pytest.mark.parametrize("geom", GEOMETRIES, ids=["S16_T4", "S256_T64"])
@pytest.mark.parametrize("where", ["tile_first", "tile_last", "superchunk_first", "superchunk_last"])
def test_rejection_at_tile_and_superchunk_edges(geom, where):
    """A draw that refuses its first attempt, so that its second attempt starts inside it, as the first and the last draw of a tile and
    of a superchunk."""
    S, T = geom["_superchunk"], geom["_tile"]
    index = {"tile_first": T, "tile_last": 2 * T - 1, "superchunk_first": S, "superchunk_last": S - 1}[where]
    lam = np.full(2 * S + 3, 86.0)
    seed = pr.find_seed(lam, pr.rejected_at(index), limit=1000)
    assert seed is not None
    _, info = _check(seed, lam, **geom)
    assert info["undecided"] == 0


@pytest.mark.parametrize("geom", GEOMETRIES, ids=["S16_T4", "S256_T64"])
@pytest.mark.parametrize("accept", [True, False], ids=["slow_accept", "slow_reject"])
def test_slow_test_at_the_last_draw_of_a_tile(geom, accept):
    S, T = geom["_superchunk"], geom["_tile"]
    lam = np.full(S + 2, 86.0)
    seed = pr.find_seed(lam, pr.slow_at(T - 1, accept), limit=1000)
    assert seed is not None
    _check(seed, lam, **geom)


@pytest.mark.parametrize("geom", GEOMETRIES, ids=["S16_T4", "S256_T64"])
def test_long_mult_draw_across_a_superchunk_end(geom):
    S = geom["_superchunk"]
    lam = np.full(2 * S, 86.0)
    lam[S - 1] = 9.9
    seed = pr.find_seed(lam, pr.mult_at_least(S - 1, 12), limit=1000)
    assert seed is not None
    got, _ = _check(seed, lam, **geom)
    assert got[S - 1] >= 12


@pytest.mark.parametrize("geom", GEOMETRIES, ids=["S16_T4", "S256_T64"])
def test_zero_rates_across_a_tile_end_and_at_a_superchunk_end(geom):
    S, T = geom["_superchunk"], geom["_tile"]
    lam = np.full(2 * S + 1, 86.0)
    lam[T - 2:T + 2] = 0.0  # a run across the end of tile 0
    lam[S - 1] = 0.0  # superchunk 0 ends in a draw that consumes nothing
    lam[2 * S - 3:2 * S] = 0.0  # and superchunk 1 in three
    got, _ = _check(11, lam, **geom)
    assert not got[lam == 0.0].any()
    _check(12, np.zeros(S + 3), **geom)  # nothing is consumed at all


def test_window_overflow_is_recovered_by_the_walk_and_reported():
    """W = 2: the path leaves the window at the first refused attempt of a superchunk.  The restatement says in which superchunks."""
    S, T, W = 16, 4, 2
    lam = np.full(3 * S + 5, 86.0)
    seed, leaves = None, 0
    for s in range(50):
        leaves = sum(w["leaves"] for w in pr.windows(pr.raw_for(s, lam), lam, S, W))
        if 1 <= leaves < 4:  # at least one superchunk by the walk and one by the tables
            seed = s
            break
    assert seed is not None
    _, info = _check(seed, lam, _superchunk=S, _tile=T, _window=W)
    assert info["recovered"] == leaves and info["undecided"] == 0


def test_force_walk_gives_the_same_bits():
    lam = _rates(3 * 256 + 5)
    a, ia = _check(31, lam, _superchunk=256, _tile=64)
    b, ib = _check(31, lam, _superchunk=256, _tile=64, _force_walk=True)
    assert a.tobytes() == b.tobytes() and ia["consumed"] == ib["consumed"] and ib["recovered"] == 0


def test_same_bits_for_every_geometry_and_from_run_to_run():
    """S in {16, 256, production}, W in {8, production}, T in {4, 64} (T = 64 only where S is a multiple of it), twice each."""
    rng = np.random.default_rng(8)
    lam = np.concatenate([np.full(600, 86.0), rng.uniform(0.0, 10.0, 100), rng.uniform(10.0, 3.0e5, 100), np.zeros(30)])
    rng.shuffle(lam)
    first = None
    for S in (16, 256, 0):
        for W in (8, 0):
            for T in (4, 64):
                if S == 16 and T == 64:
                    continue
                for _ in range(2):
                    got, info = _check(2718, lam, _superchunk=S, _window=W, _tile=T)
                    first = got if first is None else first
                    assert got.tobytes() == first.tobytes() and info["undecided"] == 0


def test_forced_undecided_request_is_drawn_by_numpy_and_flagged():
    _, info = _check(5, np.full(300, 86.0), _guard=1.0, _superchunk=256, _tile=64)
    assert info["undecided"] == 1 and info["consumed"] is None
    _, info = _check(5, np.full(300, 3.0), _guard=1.0, _superchunk=256, _tile=64)  # prod > enlam
    assert info["undecided"] == 1


def test_undecided_nodes_off_the_path_do_not_flag_the_call():
    """A guard band of 1e-5 (absolute 1e-5 * 950 at 86: a percent of the slow tests) with a window that covers every excess the 32 draws can
    reach: the restatement finds a seed whose window holds undecided nodes and whose path holds none -- the call is not flagged -- and one
    whose path holds one -- it is."""
    S, T, W, guard = 32, 4, 64, 1.0e-5
    lam = np.full(S, 86.0)
    clean = dirty = None
    for seed in range(100000):
        w = pr.windows(pr.raw_for(seed, lam), lam, S, W, guard)[0]
        assert not w["leaves"]
        if clean is None and w["off_path"] > 0 and not w["on_path"]:
            clean = seed
        if dirty is None and w["on_path"]:
            dirty = seed
        if clean is not None and dirty is not None:
            break
    if clean is None:
        pytest.skip("no seed below 1e5 has undecided nodes in the window and none on the path")
    _, info = _check(clean, lam, _superchunk=S, _tile=T, _window=W, _guard=guard)
    assert info["undecided"] == 0 and info["recovered"] == 0
    assert dirty is not None
    _, info = _check(dirty, lam, _superchunk=S, _tile=T, _window=W, _guard=guard)
    assert info["undecided"] == 1


@pytest.mark.parametrize("bad", [-1.0, float("nan"), 1.0e19])
def test_invalid_rate_raises_numpys_error(bad):
    import torch

    from pyimcom_amd import noiselayers as nl

    lam = np.full(100, 86.0)
    lam[57] = bad
    with pytest.raises(ValueError) as want:
        np.random.default_rng(1).poisson(lam=lam)
    for arg in (lam, torch.from_numpy(lam).to(DEV)):
        with pytest.raises(ValueError) as got:
            nl.poisson(1, arg)
        assert str(got.value) == str(want.value)
    with pytest.raises(TypeError):
        nl.poisson(np.random.MT19937(1), np.full(4, 86.0))


def test_c_entries_refuse_bad_arguments():
    import ctypes as C

    from pyimcom_amd import _lib

    info = np.zeros(4, dtype=np.uint64)
    for name in ("imcom_pcg64_poisson", "imcom_pcg64_poisson_ex", "imcom_nstar_layer"):
        args = [0.0 if t is C.c_double else (None if t is C.c_void_p else 0) for t in _lib.SIGNATURES[name]]
        assert getattr(_lib.lib, name)(*args) == -1 and "null context" in _lib.lib.imcom_last_error().decode()
    ctx = _lib.default_context()
    lam, out = np.full(8, 86.0), np.zeros(8, dtype=np.int64)
    call = lambda count, *ex: _lib.lib.imcom_pcg64_poisson_ex(ctx.handle, 1, 2, 3, 4, 0, 0, _lib.ptr(lam), count, _lib.ptr(out), _lib.ptr(info), _lib.MEM_HOST, *ex)  # noqa: E731
    assert call(-1, 0, 0, 0, -1.0, 0) == -1
    assert call(8, 16, 0, 5, -1.0, 0) == -1  # S no multiple of T
    assert call(8, 0, 1, 0, -1.0, 0) == -1  # window below 2
    assert call(8, 0, 0, 0, 2.0, 0) == -1
    lam[3] = -2.0
    out[:] = -7
    assert call(8, 0, 0, 0, -1.0, 0) == -1 and info[3] == 1 and np.all(out == -7)  # an invalid rate: nothing is written
    ws, scratch = C.c_long(0), C.c_long(0)
    assert _lib.lib.imcom_pcg64_poisson_sizes(4088 * 4088, C.byref(ws), C.byref(scratch)) == 0 and 0 < scratch.value < ws.value < 1 << 28
    assert _lib.lib.imcom_pcg64_poisson_sizes(-1, C.byref(ws), C.byref(scratch)) == -1


def test_state_advance_offset_and_generator_argument():
    from pyimcom_amd import noiselayers as nl

    lam = _rates(500).reshape(20, 25)
    _check(77, lam, offset=12345)
    _check(77, lam, offset=(1 << 64) + 3)
    gen, ref = np.random.default_rng(9), np.random.default_rng(9)
    gen.integers(0, 10, dtype=np.uint32)  # (leaves a cached 32-bit half, which the draws do not touch)
    ref.integers(0, 10, dtype=np.uint32)
    got = nl.poisson(gen, lam)
    assert got.tobytes() == ref.poisson(lam=lam).tobytes() and gen.bit_generator.state == ref.bit_generator.state
    assert gen.standard_normal() == ref.standard_normal()


def test_device_input_and_device_output():
    import torch

    from pyimcom_amd import noiselayers as nl

    lam = _rates(700).reshape(7, 100)
    want, _ = _numpy(3, lam)
    got = nl.poisson(3, torch.from_numpy(lam).to(DEV))
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.int64 and got.shape == (7, 100)
    assert got.cpu().numpy().tobytes() == want.tobytes()
    got = nl.poisson(3, lam, device=DEV)
    assert got.is_cuda and got.cpu().numpy().tobytes() == want.tobytes()
    got = nl.poisson(3, torch.from_numpy(lam.astype(np.float32)).to(DEV))  # (86, 3 and 0 are exact in float32)
    assert got.cpu().numpy().tobytes() == want.tobytes()


def _layer_want(brightness, tot_int, bg, q, idsca):
    rng = np.random.default_rng(1000000 * (18 * q + idsca[1]) + idsca[0])
    lam = brightness * tot_int + bg
    _lam = np.clip(lam, 0, None)
    draws = rng.poisson(lam=_lam)
    return draws, (draws - _lam + lam - bg).astype(np.float32), _lam


def test_nstar_layer_against_numpys_statements_and_the_golden():
    import torch

    from pyimcom_amd import inject
    from pyimcom_amd import noiselayers as nl

    rng = np.random.default_rng(6)
    brightness = rng.normal(2.0e-4, 4.0e-4, (64, 64))  # a third of the pixels negative: lam < 0 there, _lam = 0
    _, want, _lam = _layer_want(brightness, 2.0e5, 86.0, 3, (1234, 5))
    assert (_lam == 0).sum() > 100
    got = inject.nstar_layer(brightness, 2.0e5, 86.0, 3, (1234, 5))
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.tobytes() == want.tobytes()
    assert nl.last_poisson_info["undecided"] == 0
    got = inject.nstar_layer(torch.from_numpy(brightness).to(DEV), 2.0e5, 86.0, 3, (1234, 5), device_out=True)
    assert got.is_cuda and got.dtype == torch.float32 and got.cpu().numpy().tobytes() == want.tobytes()
    g = np.load(os.path.join(ROOT, "tests", "golden", "nstar.npz"))
    for k, string in enumerate(g["strings"].tolist()):
        res, tot_int, bg, q = inject.parse_nstar(string)
        got = inject.nstar_layer(torch.from_numpy(g[f"brightness{k}"]).to(DEV), tot_int, bg, q, tuple(int(v) for v in g["idsca"][k]))
        assert got.tobytes() == g[f"layer{k}"].tobytes(), k


def test_production_frame():
    """One 4088^2 frame: lam = 86 + 2e5 * (Gaussian spots at a 117-pixel pitch), the int64 draws and the float32 layer."""
    import torch

    from pyimcom_amd import inject
    from pyimcom_amd import noiselayers as nl

    n, q, idsca = 4088, 3, (4321, 7)
    x = np.arange(n, dtype=np.float64)
    prof = np.exp(-0.5 * ((x[:, None] - np.arange(58.5, n, 117.0)[None, :]) / 1.6) ** 2).sum(axis=1)
    brightness = prof[:, None] * prof[None, :] / (2 * np.pi * 1.6**2)
    draws, want, _lam = _layer_want(brightness, 2.0e5, 86.0, q, idsca)
    assert _lam.max() > 1.0e4
    seed = 1000000 * (18 * q + idsca[1]) + idsca[0]
    got, info = nl.poisson(seed, torch.from_numpy(_lam).to(DEV), return_info=True)
    assert info["undecided"] == 0, info
    assert torch.equal(got, torch.from_numpy(draws).to(DEV)), info
    assert 2.3 < info["consumed"] / n**2 < 2.4
    del got
    layer = inject.nstar_layer(torch.from_numpy(brightness).to(DEV), 2.0e5, 86.0, q, idsca, device_out=True)
    assert layer.dtype == torch.float32 and torch.equal(layer, torch.from_numpy(want).to(DEV))
