#!/usr/bin/env python3
"""Time the noise layers on the device (pyimcom_amd.noiselayers; INTEGRATION.md seam 13).  White: one frame of nside^2 normal draws, host
out and device out, with the kernels' own event times (zig_map / zig_chain / zig_emit: the tile tables, the walk over the tiles, the
values), and numpy's time for the same frame on the host this runs on.  1/f: one ``noise_1f_frame``, host out and device out, split into
the draws (with the walk over the tiles on its own), the tail values formed on the host, and the transform (the two DFT steps; the sums
and the placement), and the time of the reference's statements in numpy (tests/noise1f_reference.py) on this host.  One JSON line, also
written to profiles/noise_bench.json.

    python tools/bench_noise.py [--nside 4088] [--reps 5] [--warmup 2] [--no-host]
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nside", type=int, default=4088)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    import torch

    from pyimcom_amd import _lib, noiselayers as nl

    seed, dev = 1000000 * (18 * 2 + 5) + 1234, "cuda:0"
    ctx = _lib.default_context()
    res = {"what": "white_noise_frame", "nside": args.nside, "draws": args.nside**2, "device": torch.cuda.get_device_name(0), "source": _lib.source_sha16()}

    def timed(device):
        ts = []
        for i in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            nl.white_noise_frame(seed, args.nside, device=device)
            torch.cuda.synchronize()
            if i >= args.warmup:
                ts.append(time.perf_counter() - t0)
        return float(np.median(ts))

    res["ms_host_out"] = 1e3 * timed(None)
    res["ms_device_out"] = 1e3 * timed(dev)
    res["info"] = dict(nl.last_info)
    ctx.profile_enable(1)
    ctx.profile_reset()
    nl.white_noise_frame(seed, args.nside, device=dev)
    torch.cuda.synchronize()
    res["kernel_ms"] = {k: ctx.profile_get(k)[0] for k in ("zig_map", "zig_chain", "zig_emit")}  # chain: the walk over the tiles
    ctx.profile_enable(0)
    if not args.no_host:
        t0 = time.perf_counter()
        np.random.default_rng(seed).normal(loc=0.0, scale=1.0, size=(args.nside, args.nside))
        res["numpy_s"] = time.perf_counter() - t0

    # the 1/f frame
    f1 = {"what": "noise_1f_frame", "len": 8192 * 128, "nch": 32, "w": 128, "draws": 64 * 8192 * 128}

    def timed_1f(device_out):
        ts = []
        for i in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            nl.noise_1f_frame(seed, device_out=device_out)
            torch.cuda.synchronize()
            if i >= args.warmup:
                ts.append(time.perf_counter() - t0)
        return float(np.median(ts))

    f1["ms_host_out"] = 1e3 * timed_1f(False)
    f1["ms_device_out"] = 1e3 * timed_1f(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    normals = nl.standard_normal(np.random.PCG64(seed), (64, 8192 * 128), device=dev)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    amp = nl.noise_1f_amp(8192 * 128)
    t2 = time.perf_counter()
    nl.noise_1f(normals, amp, 32, 128)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    f1["ms_draws"], f1["ms_amp_host"], f1["ms_transform"], f1["info"] = 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2), dict(nl.last_info)
    ctx.profile_enable(1)
    ctx.profile_reset()
    nl.noise_1f_frame(seed, device_out=True)
    torch.cuda.synchronize()
    f1["kernel_ms"] = {k: ctx.profile_get(k)[0] for k in ("zig_map", "zig_chain", "zig_emit", "n1f_transform", "n1f_place")}
    ctx.profile_enable(0)
    del normals
    if not args.no_host:
        sys.path.insert(0, ROOT)
        from tests import noise1f_reference as ref

        t0 = time.perf_counter()
        g = ref.draws(seed, 8192 * 128, 32)
        t1 = time.perf_counter()
        ref.restated(g, ref.amp_of(8192 * 128), 128)
        f1["numpy_draws_s"], f1["numpy_transform_s"] = t1 - t0, time.perf_counter() - t1
    res["noise_1f"] = f1
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "noise_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
