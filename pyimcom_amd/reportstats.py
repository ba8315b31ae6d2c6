"""The statistics of the validation report on the device: the layer percentiles of ``LayerReport.build`` (reference
src/pyimcom/diagnostics/layer_diagnostics.py:24-64 and 102-177) and the ring profiles and the two histograms of ``gen_dynrange_data``
(src/pyimcom/diagnostics/dynrange.py:140-163 and 211-238).  The binding (seam 12):

    pcarray = pyimcom_amd.reportstats.layer_percentiles(frames_by_block, ns, d, nblock, pctiles)         # LayerReport.build 105-177
    tables = pyimcom_amd.reportstats.dynrange_tables(blocks, rpix, bd)                                  # gen_dynrange_data 140-163, 211-238

The reference gathers a layer of the whole mosaic into one array, sorts it out of core and reads 13 percentiles; it histograms the SIGMA
and EFFCOVER maps with 200 full-image comparisons a block and collects star neighbourhoods ring by ring with ``np.concatenate``.  All of
it is order statistics and integer counts.  csrc/quantiles.hip counts; ``StreamingQuantiles`` is a radix select whose data arrives in
chunks and is fed once per pass (three passes for float32), for up to 64 segments and 32 ranks per segment at once; nothing is rounded
on the device, so every number equals numpy's.

What stays on the host, in numpy scalars of the types the reference has there: the ranks of a percentile and the interpolation between
the two order statistics that bracket it (``_percentiles_and_delete`` 52-57; ``np.percentile``'s linear rule, 238), and the table of the
65 536 codes of a compressed map (142-147, 155-160: the reference's own expression and comparisons, evaluated once per code instead of
once per pixel).  Star positions (healpy, the WCS), FITS, the figures and the LaTeX are the caller's."""

import ctypes as C

import numpy as np

from ._dev import DEVICE, bound_context, device_of, is_torch, np_dtype, staged, to_host
from ._lib import MEM_DEVICE, check, lib, ptr

__all__ = ["StreamingQuantiles", "layer_percentiles", "dynrange_tables", "percentile_ranks", "percentile_from_order_statistics", "code_bin_table",
           "coded_map_histogram", "LAYER_PCTILES", "RING_PCTILES", "MAX_SEGMENTS", "MAX_RANKS"]

MAX_SEGMENTS, MAX_RANKS = 64, 32
LAYER_PCTILES = [0, 0.01, 0.1, 1, 5, 25, 50, 75, 95, 99, 99.9, 99.99, 100]  # layer_diagnostics.py:103
RING_PCTILES = [1, 5, 25, 50, 75, 95, 99]  # dynrange.py:237


class StreamingQuantiles:
    """Exact order statistics of ``n_segments`` multisets of float32 / float64 values that arrive in chunks.

        sq = StreamingQuantiles(2, np.float32)
        stats = sq.run(feed, ranks)            # feed(sq) adds every chunk; it is called once per pass with the same data

    or pass by pass: feed, ``end_pass()``, after the first pass ``counts()`` and ``set_ranks(ranks)``, feed again ... until ``end_pass``
    returns 0, then ``order_statistics()``.  NaNs sort last (a rank among them gives NaN), -0.0 and 0.0 are one value.  A pass that was fed
    another number of elements (or of NaNs) in a segment than the first raises at ``end_pass`` and can be fed again; ``reset`` starts over.
    Torch tensors on the device are read in place (a 2-D view with unit column stride too), numpy arrays are uploaded."""

    def __init__(self, n_segments, dtype=np.float32, device=None, n_ranks=MAX_RANKS, ctx=None):
        import torch

        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.float32, np.float64):
            raise TypeError(f"StreamingQuantiles: float32 or float64, not {self.dtype}")
        self.S, self.R = int(n_segments), int(n_ranks)
        self.device = torch.device(device or DEVICE)
        self.ctx = bound_context(self.device, ctx)
        sz = (C.c_long * 4)()
        check(lib.imcom_quant_sizes(self.S, self.R, int(self.dtype == np.float64), sz))
        self.passes = int(sz[1])
        self._state = torch.empty(int(sz[0]) // 8, dtype=torch.int64, device=self.device)
        self._h = C.c_void_p()
        check(lib.imcom_quant_begin(self.ctx.handle, self.S, self.R, int(self.dtype == np.float64), ptr(self._state), self._state.numel() * 8, C.byref(self._h)))
        self._nranks = 0

    def _values(self, a):
        return staged(a, self.device, (self.dtype,), f"StreamingQuantiles of {self.dtype}: a chunk of {{dtype}}", layout="any")

    def add(self, values, segment=0, segment_ids=None):
        """A chunk: every element into ``segment``, or element i into ``segment_ids[i]`` (uint8 / int32, same shape)."""
        import torch

        t = self._values(values)
        bound_context(ctx=self.ctx)
        if segment_ids is not None:
            ids = staged(segment_ids, self.device, layout="any")
            if ids.dtype not in (torch.uint8, torch.int32) or ids.shape != t.shape:
                raise TypeError(f"segment ids: uint8 or int32 of shape {tuple(t.shape)}, not {ids.dtype} {tuple(ids.shape)}")
            t, ids = t.contiguous(), ids.contiguous()
            check(lib.imcom_quant_add_flat(self.ctx.handle, self._h, ptr(t), ptr(ids), int(ids.dtype == torch.int32), t.numel(), MEM_DEVICE))
            return
        if t.numel() == 0:
            return
        if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]:
            rows, cols, pitch = t.shape[0], t.shape[1], t.stride(0)
        else:
            t = t.contiguous()
            rows, cols, pitch = 1, t.numel(), t.numel()
        check(lib.imcom_quant_add_2d(self.ctx.handle, self._h, int(segment), ptr(t), rows, cols, pitch, MEM_DEVICE))

    def add_constant(self, segment, value, count):
        """``count`` copies of ``value`` (rounded to the accumulator's type) without data."""
        bound_context(ctx=self.ctx)
        check(lib.imcom_quant_add_constant(self.ctx.handle, self._h, int(segment), float(self.dtype.type(value)), int(count)))

    def add_star_rings(self, frame, x, y, rpix):
        """dynrange.py:216-228: the pixels around the stars at (``x``, ``y``) (float64) of the square ``frame``, ring j into segment j."""
        t = self._values(frame)
        if t.dim() != 2 or t.shape[0] != t.shape[1] or t.stride(1) != 1:
            raise ValueError(f"add_star_rings: a square frame with unit column stride, not {tuple(t.shape)}")
        xs, ys = (staged(np.asarray(to_host(v), dtype=np.float64), self.device) for v in (x, y))
        if xs.shape != ys.shape or xs.dim() != 1:
            raise ValueError("add_star_rings: x and y are 1-D arrays of one length")
        bound_context(ctx=self.ctx)
        check(lib.imcom_quant_add_rings(self.ctx.handle, self._h, ptr(t), t.shape[0], t.stride(0), ptr(xs), ptr(ys), xs.numel(), int(rpix), MEM_DEVICE))

    def end_pass(self):
        """Ends the pass that was fed; returns the number of passes still to feed."""
        left = C.c_int(0)
        bound_context(ctx=self.ctx)
        check(lib.imcom_quant_end_pass(self.ctx.handle, self._h, C.byref(left)))
        return left.value

    def counts(self):
        """(elements, NaNs among them) per segment, int64 arrays, once the first pass has ended."""
        total, nans = np.zeros(self.S, dtype=np.int64), np.zeros(self.S, dtype=np.int64)
        check(lib.imcom_quant_counts(self.ctx.handle, self._h, ptr(total), ptr(nans)))
        return total, nans

    def set_ranks(self, ranks):
        """ranks [n_segments, k <= n_ranks]: 0-based ranks in ascending order, -1 for a slot not used (between pass 1 and pass 2)."""
        r = np.asarray(ranks, dtype=np.int64)
        if r.ndim != 2 or r.shape[0] != self.S or r.shape[1] > self.R:
            raise ValueError(f"set_ranks: an array [{self.S}, <= {self.R}], not {r.shape}")
        full = np.full((self.S, self.R), -1, dtype=np.int64)
        full[:, :r.shape[1]] = r
        bound_context(ctx=self.ctx)
        check(lib.imcom_quant_set_ranks(self.ctx.handle, self._h, ptr(full)))
        self._nranks = r.shape[1]

    def order_statistics(self):
        """[n_segments, k] of the accumulator's type after the last pass: the values at the ranks that were set."""
        out = np.zeros((self.S, self.R), dtype=self.dtype)
        check(lib.imcom_quant_results(self.ctx.handle, self._h, ptr(out)))
        return out[:, :self._nranks].copy()

    def run(self, feed, ranks):
        """Every pass: ``feed(self)`` adds all the data.  ``ranks``: an array for ``set_ranks`` or a function of ``counts()`` that makes one."""
        for p in range(self.passes):
            feed(self)
            self.end_pass()
            if p == 0:
                self.set_ranks(ranks(*self.counts()) if callable(ranks) else ranks)
        return self.order_statistics()

    def reset(self):
        bound_context(ctx=self.ctx)
        check(lib.imcom_quant_reset(self.ctx.handle, self._h))
        self._nranks = 0

    def close(self):
        if self._h:
            lib.imcom_quant_free(self.ctx.handle, self._h)
            self._h = C.c_void_p()
            self._state = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- layer percentiles (layer_diagnostics.py) ----
def _layer_position(nsize, pct):
    """layer_diagnostics.py:52-56: (p1, frac) of one percentile of ``nsize`` sorted values."""
    pos = (nsize - 1) * pct / 100.0
    p1 = max(int(np.floor(pos)), 0)
    if p1 >= nsize - 1:
        p1 = nsize - 2
    return p1, np.clip(pos - p1, 0.0, 1.0)


def layer_percentiles(frames_by_block, ns, d, nblock, pctiles=LAYER_PCTILES):
    """``pcarray`` [nlayers, len(pctiles)] float32 of LayerReport.build (105-177).  ``frames_by_block[(ibx, iby)]``: the float32 frames
    [nlayers, ns + 2 d, ns + 2 d] of a block, on the device (``BlockMaps.report_views``) or as a numpy array; a block that is missing or
    None counts as ``ns``^2 zeros per layer, as the file the reference does not find (114, 122, 133-134).  Every layer is a segment of one
    accumulator; the frames are read in place, three times."""
    ns, d, nblock = int(ns), int(d), int(nblock)
    nsize = (ns * nblock) ** 2
    if nsize < 2:
        raise ValueError("layer_percentiles: fewer than 2 values (the reference reads arr[p1 + 1] out of range)")
    have = {k: v for k, v in frames_by_block.items() if v is not None and 0 <= k[0] < nblock and 0 <= k[1] < nblock}
    if not have:
        raise ValueError("layer_percentiles: no block")
    nlayers = {int(v.shape[0]) for v in have.values()}
    if len(nlayers) != 1:
        raise ValueError(f"layer_percentiles: blocks with {sorted(nlayers)} layers")
    nlayers = nlayers.pop()
    for k, v in have.items():
        if tuple(v.shape[1:]) != (ns + 2 * d, ns + 2 * d):
            raise ValueError(f"layer_percentiles: block {k} has frames {tuple(v.shape[1:])}, not {ns} + 2 x {d} on a side")
    missing = nblock * nblock - len(have)
    where = [_layer_position(nsize, p) for p in pctiles]
    ranks = sorted({p1 for p1, _ in where} | {p1 + 1 for p1, _ in where})
    if len(ranks) > MAX_RANKS:
        raise ValueError(f"layer_percentiles: {len(pctiles)} percentiles need {len(ranks)} order statistics, served are {MAX_RANKS}")
    pcarray = np.zeros((nlayers, len(pctiles)), dtype=np.float32)
    first = next(iter(have.values()))
    device = device_of(first)
    for l0 in range(0, nlayers, MAX_SEGMENTS):
        nl = min(MAX_SEGMENTS, nlayers - l0)
        sq = StreamingQuantiles(nl, np.float32, device=device, n_ranks=len(ranks))

        def feed(sq):
            for v in have.values():
                for s in range(nl):
                    sq.add(v[l0 + s][d:d + ns, d:d + ns], segment=s)
            if missing:
                for s in range(nl):
                    sq.add_constant(s, 0.0, missing * ns * ns)

        a = sq.run(feed, np.tile(np.asarray(ranks, dtype=np.int64), (nl, 1)))
        sq.close()
        at = {r: i for i, r in enumerate(ranks)}
        for s in range(nl):
            for k, (p1, frac) in enumerate(where):
                with np.errstate(invalid="ignore", over="ignore"):
                    pcarray[l0 + s, k] = (1 - frac) * a[s, at[p1]] + frac * a[s, at[p1 + 1]]  # (57: float64 arithmetic, stored as float32)
    return pcarray


# ---- np.percentile's linear rule from two order statistics (dynrange.py:238) ----
def percentile_ranks(n, q, dtype=np.float32):
    """(previous rank, next rank, gamma) of ``np.percentile(a, q)`` (method "linear") for ``a`` of ``n`` >= 1 values of ``dtype`` and a Python
    number ``q``: numpy divides q by 100 in the array's type and forms the virtual index (n - 1) q in it."""
    t = np.dtype(dtype).type
    quant = np.true_divide(q, t(100))
    virtual = (n - 1) * quant
    prev = np.floor(virtual)
    nxt = prev + 1
    gamma = virtual - prev
    if virtual >= n - 1:
        prev = nxt = n - 1
        gamma = virtual - t(-1)  # (numpy's indexes are -1 there; the two values are equal, gamma multiplies 0)
    if virtual < 0:
        prev = nxt = 0
        gamma = virtual - t(0)
    return int(prev), int(nxt), t(gamma)


def percentile_from_order_statistics(a, b, gamma, any_nan=False):
    """numpy's ``_lerp`` of the order statistics ``a`` <= ``b`` (scalars of the array's type) with weight ``gamma``; NaN if the data has one."""
    t = type(gamma)
    if any_nan:
        return t(np.nan)
    a, b = t(a), t(b)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = b - a
        out = a + diff * gamma
        if gamma >= 0.5:
            out = b - diff * (1 - gamma)
    return t(out)


# ---- histograms of coded maps (dynrange.py:142-163) ----
def code_bin_table(values, width, nbins):
    """The bin of each of the 65 536 codes: ``values`` [65536] is the reference's expression on every code (indexed by the code's bit
    pattern).  Entry j < nbins where ``values / width >= j`` and ``values / width < j + 1`` (146-147), nbins where only
    ``values >= width * nbins`` (150: off scale high), 128 + j where both hold, 255 where neither does (a NaN, a value below zero)."""
    if not 1 <= nbins <= 127:
        raise ValueError("code_bin_table: 1 .. 127 bins")
    values = np.asarray(values)
    table = np.full(65536, 255, dtype=np.uint8)
    with np.errstate(all="ignore"):
        for j in range(nbins):
            table[np.logical_and(values / width >= j, values / width < j + 1)] = j
        high = values >= width * nbins
    both = high & (table < nbins)
    table[high & ~both] = nbins
    table[both] += 128
    return table


def _all_codes(dtype):
    """Every code of a 16-bit integer type, indexed by its bit pattern."""
    dtype = np.dtype(dtype)
    if dtype not in (np.int16, np.uint16):
        raise TypeError(f"a coded map is int16 or uint16, not {dtype}")
    return np.arange(65536, dtype=np.uint32).astype(np.uint16).view(dtype)


def coded_map_histogram(codes, table, nbins, ctx=None):
    """int64 [nbins + 1]: how many codes of the 2-D view ``codes`` (int16 / uint16; a device tensor is read in place) fall into each bin of
    ``table`` (``code_bin_table``); the last entry counts "off scale high"."""
    import torch

    t = staged(codes, device_of(codes), None if is_torch(codes) else (np.int16, np.uint16), "a coded map is int16 or uint16, not {dtype}", layout="any")
    if t.dtype not in (torch.int16, torch.uint16) or t.dim() != 2:
        raise TypeError(f"a coded map is a 2-D int16 or uint16 array, not {t.dtype} {tuple(t.shape)}")
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    ctx = bound_context(t.device, ctx)
    tab = staged(np.asarray(table, dtype=np.uint8), t.device)
    out = torch.zeros(nbins + 1, dtype=torch.int64, device=t.device)
    check(lib.imcom_codehist(ctx.handle, ptr(t), t.shape[0], t.shape[1], t.stride(0), ptr(tab), int(nbins), ptr(out), MEM_DEVICE))
    return out.cpu().numpy()


N_NOISE, D_NOISE, N_NEFF, D_NEFF = 100, 0.02, 100, 0.1  # dynrange.py:68-77


def dynrange_tables(blocks, rpix, bd, nscale=1):
    """The numbers of gen_dynrange_data's three files.  ``blocks``: one dict per block file the reference would find, with ``starmap``
    (float32 [n, n], the injected-star layer), ``x``, ``y`` (float64 pixel positions of its stars, 177-191: the caller's healpy and WCS),
    and optionally ``sigma`` / ``neff`` = (codes [n, n] int16 or uint16, bels): the SIGMA and EFFCOVER maps as compressed and
    ``HDU_to_bels`` of their headers.  ``rpix`` rings (113), ``bd`` the padding the histograms leave out (112).  Returns a dict:
    ``dynrange`` float64 [rpix, 9] = ring, count, the percentiles 1, 5, 25, 50, 75, 95, 99 (235-239); ``countnoise``, ``countneff``
    float64 [100, 2] (70-71, 76-77, 145-148, 158-161) and ``noise_header``, ``neff_header`` = (largest count, percent off scale high)
    (252, 256)."""
    rpix, bd = int(rpix), int(bd)
    if not 1 <= rpix <= MAX_SEGMENTS:
        raise ValueError(f"dynrange_tables: 1 .. {MAX_SEGMENTS} rings, not {rpix}")
    countnoise = np.zeros((N_NOISE, 2))
    countnoise[:, 0] = D_NOISE * np.linspace(0.5, N_NOISE - 0.5, N_NOISE)
    countneff = np.zeros((N_NEFF, 2))
    countneff[:, 0] = D_NEFF * np.linspace(0.5, N_NEFF - 0.5, N_NEFF)
    tnoise = tnoise_gt = tneff = tneff_gt = 0.0
    tables = {}
    for b in blocks:
        n = int(b["starmap"].shape[-1])
        for key, width, nb, count in (("sigma", D_NOISE, N_NOISE, countnoise), ("neff", D_NEFF, N_NEFF, countneff)):
            if b.get(key) is None:
                continue
            codes, bels = b[key]
            dt = np_dtype(codes)
            if (key, dt, bels) not in tables:
                with np.errstate(all="ignore"):
                    vals = 10 ** (0.5 * bels * _all_codes(dt)) if key == "sigma" else 10 ** (bels * _all_codes(dt) * nscale)  # (142-144, 155-157)
                tables[(key, dt, bels)] = code_bin_table(vals, width, nb)
            h = coded_map_histogram(codes[bd:n - bd, bd:n - bd], tables[(key, dt, bels)], nb)
            count[:, 1] = count[:, 1] + h[:nb]
            if key == "sigma":
                tnoise, tnoise_gt = tnoise + (n - 2 * bd) ** 2, tnoise_gt + h[nb]
            else:
                tneff, tneff_gt = tneff + (n - 2 * bd) ** 2, tneff_gt + h[nb]
    first = blocks[0]["starmap"]
    sq = StreamingQuantiles(rpix, np.float32, device=device_of(first), n_ranks=2 * len(RING_PCTILES))

    def feed(sq):
        for b in blocks:
            sq.add_star_rings(b["starmap"], b["x"], b["y"], rpix)

    def ranks(total, nans):
        out = np.full((rpix, 2 * len(RING_PCTILES)), -1, dtype=np.int64)
        for j in range(rpix):
            if total[j] > 0:
                for k, q in enumerate(RING_PCTILES):
                    out[j, 2 * k], out[j, 2 * k + 1], _ = percentile_ranks(int(total[j]), q, np.float32)
        return out

    a = sq.run(feed, ranks)
    total, nans = sq.counts()
    sq.close()
    dyn = np.zeros((rpix, 2 + len(RING_PCTILES)))
    for j in range(rpix):
        dyn[j, 0], dyn[j, 1] = j, total[j]
        for k, q in enumerate(RING_PCTILES):
            if total[j] == 0:
                dyn[j, 2 + k] = np.nan  # (no values: np.percentile raises there)
            else:
                g = percentile_ranks(int(total[j]), q, np.float32)[2]
                dyn[j, 2 + k] = percentile_from_order_statistics(a[j, 2 * k], a[j, 2 * k + 1], g, nans[j] > 0)
    with np.errstate(all="ignore"):
        return {"dynrange": dyn, "countnoise": countnoise, "countneff": countneff,
                "noise_header": (np.amax(countnoise[:, 1]), 100 * tnoise_gt / tnoise if tnoise else np.nan),
                "neff_header": (np.amax(countneff[:, 1]), 100 * tneff_gt / tneff if tneff else np.nan)}
