#!/usr/bin/env python3
"""Time the nstar layer on the device (pyimcom_amd.inject.nstar_layer; INTEGRATION.md seam 22).  One frame of nside^2 pixels, lam = 86 + 2e5 *
(Gaussian spots at a 117-pixel pitch), brightness on the device and the float32 layer left there: wall time, the kernels' own event times
(poi_prep, poi_outputs, poi_map, poi_chain, poi_values, poi_walk), the superchunks recovered by the walk, and a sweep of the superchunk S
and the window W over the int64 draws (``noiselayers.poisson``).  In the same run the route it replaces, on the host this runs on:
download the float64 brightness, numpy's draw and formula, upload the float32 layer.  One JSON line, also written to
profiles/poisson_bench.json.

    python tools/bench_poisson.py [--nside 4088] [--reps 3] [--warmup 1] [--no-sweep]
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ("poi_prep", "poi_outputs", "poi_map", "poi_chain", "poi_values", "poi_walk")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nside", type=int, default=4088)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-sweep", action="store_true")
    args = ap.parse_args()
    import torch

    from pyimcom_amd import _lib, inject, noiselayers as nl

    n, tot_int, bg, q, idsca, dev = args.nside, 2.0e5, 86.0, 3, (4321, 7), "cuda:0"
    seed = 1000000 * (18 * q + idsca[1]) + idsca[0]
    x = np.arange(n, dtype=np.float64)
    prof = np.exp(-0.5 * ((x[:, None] - np.arange(58.5, n, 117.0)[None, :]) / 1.6) ** 2).sum(axis=1)
    brightness = torch.from_numpy(prof[:, None] * prof[None, :] / (2 * np.pi * 1.6**2)).to(dev)
    ctx = _lib.default_context()
    res = {"what": "nstar_layer", "nside": n, "draws": n * n, "tot_int": tot_int, "bg": bg, "device": torch.cuda.get_device_name(0), "source": _lib.source_sha16()}

    def timed(fn):
        ts = []
        for i in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= args.warmup:
                ts.append(time.perf_counter() - t0)
        return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts))

    res["ms_device"], res["ms_device_min"] = timed(lambda: inject.nstar_layer(brightness, tot_int, bg, q, idsca, device_out=True))
    res["info"] = dict(nl.last_poisson_info)
    ctx.profile_enable(1)
    ctx.profile_reset()
    layer = inject.nstar_layer(brightness, tot_int, bg, q, idsca, device_out=True)
    torch.cuda.synchronize()
    res["kernel_ms"] = {k: ctx.profile_get(k)[0] for k in KERNELS}
    ctx.profile_enable(0)

    def host_route():
        b = brightness.cpu().numpy()
        rng = np.random.default_rng(seed)
        lam = b * tot_int + bg
        _lam = np.clip(lam, 0, None)
        return torch.from_numpy((rng.poisson(lam=_lam) - _lam + lam - bg).astype(np.float32)).to(dev)

    res["ms_host_route"], res["ms_host_route_min"] = timed(host_route)
    res["equal_to_host_route"] = bool(torch.equal(layer, host_route()))
    if not args.no_sweep:
        lam = torch.clamp(brightness * tot_int + bg, min=0.0)
        sweep = []
        for S, W in ((2048, 384), (4096, 512), (8192, 512), (8192, 768), (8192, 1024), (16384, 1024), (32768, 1536), (65536, 2048)):
            ms, _ = timed(lambda: nl.poisson(seed, lam, _superchunk=S, _window=W))
            sweep.append({"S": S, "W": W, "ms": ms, "recovered": nl.last_poisson_info["recovered"]})
        res["sweep_int64_draws"] = sweep
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "poisson_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
