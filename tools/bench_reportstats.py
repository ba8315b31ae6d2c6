#!/usr/bin/env python3
"""Times the validation report's statistics on the device (pyimcom_amd.reportstats, INTEGRATION.md seam 12) and writes
profiles/reportstats_bench.json:

  layer_one    one layer of 4 x 4 blocks with a unique area of 2560^2 (frames of 2688^2, d = 64), 13 percentiles
  layer_all    all --layers layers of that mosaic in one accumulator
  rings        the ring table of --stars stars on one 2688^2 frame, 50 rings x 7 percentiles

Per case: the median and the spread of --reps timed runs after --warmup untimed ones (wall clock around a device synchronisation; a run
is three passes with a host step between them, so its launches cannot be bracketed by one pair of events), the bytes a select must read
at least (three reads of every float32 element) and their share of the 6.29 TB/s a float4 copy reaches on this chip.  A pass with more
than 8 live groups in a segment reads the chunk once per 8 groups, so the true traffic is higher; the figure is a floor.  Next to it the
reference's route on the host this runs on: np.sort(kind="mergesort") and the loop of layer_diagnostics.py:49-57 on --host-fraction of the
one-layer array, and the ring loop of dynrange.py:212-238 on --host-stars stars."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ROOF = 6.29e12  # bytes / s, float4 copy


def timed(fn, sync, warmup, reps):
    for _ in range(warmup):
        fn()
    sync()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        t.append(time.perf_counter() - t0)
    t = np.asarray(t)
    return {"median_s": float(np.median(t)), "min_s": float(t.min()), "max_s": float(t.max()), "reps": int(reps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--stars", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-fraction", type=float, default=1 / 16)
    ap.add_argument("--host-stars", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reportstats_bench.json"))
    a = ap.parse_args()
    import torch

    from pyimcom_amd import _lib
    from pyimcom_amd import reportstats as RS
    from tests import reportstats_reference as R

    dev = torch.device("cuda:0")
    sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731
    ns, d, nblock = 2560, 64, 4
    n = ns + 2 * d
    gen = torch.Generator(device=dev).manual_seed(1)
    frames = {(bx, by): torch.randn((a.layers, n, n), generator=gen, device=dev, dtype=torch.float32) for by in range(nblock) for bx in range(nblock)}
    res = {"device": torch.cuda.get_device_name(dev), "source_sha16": _lib.source_sha16(), "hbm_roof_bytes_per_s": HBM_ROOF, "ns": ns, "d": d, "nblock": nblock,
           "layers": a.layers, "cases": {}}
    one = {k: v[:1] for k, v in frames.items()}
    for name, f, nl in (("layer_one", one, 1), ("layer_all", frames, a.layers)):
        t = timed(lambda: RS.layer_percentiles(f, ns, d, nblock), sync, a.warmup, a.reps)
        t["elements"] = nl * (ns * nblock) ** 2
        t["bytes_read_floor"] = 3 * 4 * t["elements"]
        t["share_of_hbm_roof"] = t["bytes_read_floor"] / t["median_s"] / HBM_ROOF
        res["cases"][name] = t
        print(name, t, flush=True)
    rng = np.random.default_rng(2)
    x, y = rng.uniform(60, n - 60, a.stars), rng.uniform(60, n - 60, a.stars)
    blocks = [dict(starmap=frames[(0, 0)][0], x=x, y=y)]
    t = timed(lambda: RS.dynrange_tables(blocks, 50, 64), sync, a.warmup, a.reps)
    t["stars"], t["elements"] = a.stars, int(a.stars * 104 * 104)
    t["bytes_read_floor"] = 3 * 4 * t["elements"]
    t["share_of_hbm_roof"] = t["bytes_read_floor"] / t["median_s"] / HBM_ROOF
    res["cases"]["rings"] = t
    print("rings", t, flush=True)
    # the reference's route on this host
    m = int((ns * nblock) ** 2 * a.host_fraction)
    arr = np.random.default_rng(3).standard_normal(m).astype(np.float32)
    t0 = time.perf_counter()
    arr.sort(kind="mergesort")
    R.percentiles_of_sorted(arr, R.PCTILES)
    res["host_layer"] = {"elements": m, "fraction_of_layer_one": a.host_fraction, "seconds": time.perf_counter() - t0, "cpus": os.cpu_count()}
    sm = frames[(0, 0)][0].cpu().numpy()
    t0 = time.perf_counter()
    n_, rpix = sm.shape[-1], 50
    x_, y_ = np.meshgrid(range(n_), range(n_))
    tempvals = [np.zeros((0,), dtype=np.float32) for _ in range(rpix)]
    for i in range(a.host_stars):  # dynrange.py:216-228
        xmin, xmax = np.clip(np.floor(x[i]).astype(np.int16) - rpix - 1, 0, n_), np.clip(np.ceil(x[i]).astype(np.int16) + rpix + 1, 0, n_)
        ymin, ymax = np.clip(np.floor(y[i]).astype(np.int16) - rpix - 1, 0, n_), np.clip(np.ceil(y[i]).astype(np.int16) + rpix + 1, 0, n_)
        r = np.floor(np.sqrt((x_[ymin:ymax, xmin:xmax] - x[i]) ** 2 + (y_[ymin:ymax, xmin:xmax] - y[i]) ** 2)).astype(np.int16)
        for j in range(rpix):
            tempvals[j] = np.concatenate((tempvals[j], sm[ymin:ymax, xmin:xmax][r == j]))
    for j in range(rpix):
        for q in R.RING_Q:
            np.percentile(tempvals[j], q)
    res["host_rings"] = {"stars": a.host_stars, "fraction_of_rings": a.host_stars / a.stars, "seconds": time.perf_counter() - t0}
    print("host", res["host_layer"], res["host_rings"], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
