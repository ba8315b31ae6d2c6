#!/usr/bin/env python3
"""Times the simulated cosmic-ray masks of pyimcom_amd.simmask on the device: ``randmask`` at 4088 x 4088 for the 18 SCAs of one
observation, mask left on the device and mask copied to the host, and ``uniform`` on 2^24 draws; the median of the timed repetitions
after warm-up calls, by a host clock around work that ends in a device synchronise, and the kernels' own time from the library's event
scopes.  Next to it the time of the reference's formula for ONE mask in numpy on the host it runs on:

    g = default_rng(100000000 + obsid).uniform(size=(18, nside + 20, nside + 20))[sca - 1];  hit = g < pcut;
    good = no hit among the 3 x 3 pixels around (y + 10, x + 10)

(2.4 GB of draws at nside 4088; ``--no-host`` leaves it out).  Prints one JSON line and writes it to profiles/crmask_bench.json.

    python tools/bench_crmask.py [--reps 5] [--warmup 2] [--no-host]"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nside", type=int, default=4088)
    ap.add_argument("--obsid", type=int, default=1234)
    ap.add_argument("--pcut", type=float, default=0.002)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    import torch

    from pyimcom_amd import _lib, simmask

    ctx = _lib.default_context(0)
    nside, ndraw = args.nside, 1 << 24
    res = {"tool": "bench_crmask", "nside": nside, "obsid": args.obsid, "pcut": args.pcut, "scas": 18, "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "source_sha16": _lib.source_sha16()}

    def timed(fn, scope):
        wall, kern = [], []
        for i in range(args.warmup + args.reps):
            ctx.profile_enable(True)
            ctx.profile_reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if i >= args.warmup:
                wall.append((time.perf_counter() - t0) * 1e3)
                kern.append(ctx.profile_get(scope)[0])
            ctx.profile_enable(False)
        return statistics.median(wall), min(wall), max(wall), statistics.median(kern), out

    good = {}

    def masks(device_out):
        def run():
            for sca in range(1, 19):
                m = simmask.randmask((args.obsid, sca), args.pcut, nside=nside, device_out=device_out)
                good[sca] = m
            return m
        return run

    for name, device_out in (("device_out", True), ("host_out", False)):
        ms, lo, hi, k, _ = timed(masks(device_out), "cr_mask")
        res[f"ms_18_masks_{name}"], res[f"ms_18_masks_{name}_min"], res[f"ms_18_masks_{name}_max"] = ms, lo, hi
        res[f"ms_18_masks_{name}_kernels"] = k
    res["good_fraction_sca18"] = float(np.count_nonzero(good[18])) / nside**2
    ms, lo, hi, k, u = timed(lambda: simmask.uniform(100000000 + args.obsid, 0, ndraw, device="cuda:0"), "pcg64_uniform")
    res.update({"uniform_draws": ndraw, "ms_uniform": ms, "ms_uniform_min": lo, "ms_uniform_max": hi, "ms_uniform_kernel": k,
                "uniform_mean": float(u.mean().item())})
    if not args.no_host:
        t0 = time.perf_counter()
        W = nside + 20
        hit = np.random.default_rng(100000000 + args.obsid).uniform(size=(18, W, W))[17] < args.pcut
        t1 = time.perf_counter()
        near = np.zeros((nside, nside), dtype=bool)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                near |= hit[10 + dy:10 + dy + nside, 10 + dx:10 + dx + nside]
        t2 = time.perf_counter()
        res["s_numpy_host_one_mask"], res["s_numpy_host_one_mask_draw"] = t2 - t0, t1 - t0
        res["host_mask_equal"] = bool(np.array_equal(~near, good[18]))
        del hit
        t0 = time.perf_counter()
        np.random.default_rng(100000000 + args.obsid).uniform(size=ndraw)
        res["ms_numpy_host_uniform"] = (time.perf_counter() - t0) * 1e3
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "crmask_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
