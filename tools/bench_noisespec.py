#!/usr/bin/env python3
"""Times the noise power spectra of pyimcom_amd.noisespec on the device: 6 float32 frames of side 2560 and 6 of side 2688 resident on the
device, on the two-level route and on the dense route; the transform and the epilogue separately (the library's own event scopes) and the
whole call (events around it), the median of the timed repetitions after warm-up calls.  Next to it the reference's formula
(analysis.py:789-794) in numpy on the host for one frame.  Prints one JSON line and writes it to profiles/noisespec_bench.json.

    python tools/bench_noisespec.py [--reps 5] [--warmup 2] [--no-host]

The share of the HBM roof uses the tool's own byte count per frame: the input once, the intermediate H written and read, the half spectrum
F written and read, the output once -- what the kernels must move, not what the counters saw."""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ROOF = 8.0e12  # bytes per second, MI355X peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    import torch

    from pyimcom_amd import _lib, noisespec as ns

    dev = torch.device("cuda:0")
    ctx = _lib.default_context(0)
    res = {"tool": "bench_noisespec", "frames": args.frames, "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "source_sha16": _lib.source_sha16(), "hbm_roof_bytes_per_s": HBM_ROOF, "cases": []}
    for L in (2560, 2688):
        frames = torch.randn((args.frames, L, L), dtype=torch.float32, device=dev)
        norm = (L / 0.0390625) ** 2
        half = (L // 2 + 1) * L * 16
        bytes_frame = L * L * 4 + 4 * half + (L // 8) ** 2 * 8
        outs = {}
        for name, route in (("two_level", ns.ROUTE_TWOLEVEL), ("dense", ns.ROUTE_DENSE)):
            if int(ns._sizes(L, 1, True, 0)[0]) != ns.ROUTE_TWOLEVEL and route == ns.ROUTE_TWOLEVEL:
                continue
            whole, tr, ep = [], [], []
            for i in range(args.warmup + args.reps):
                ctx.profile_enable(True)
                ctx.profile_reset()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                outs[name] = ns.power_spectrum_2d(frames, norm, route=route, ctx=ctx)
                e1.record()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    whole.append(e0.elapsed_time(e1))
                    tr.append(ctx.profile_get("noiseps_transform")[0])
                    ep.append(ctx.profile_get("noiseps_epilogue")[0])
                ctx.profile_enable(False)
            ms = statistics.median(whole)
            res["cases"].append({"L": L, "route": name, "ms_call": ms, "ms_transform": statistics.median(tr), "ms_epilogue": statistics.median(ep),
                                 "ms_call_min": min(whole), "ms_call_max": max(whole), "ms_per_frame": ms / args.frames,
                                 "bytes_per_frame": bytes_frame, "hbm_share": bytes_frame * args.frames / (ms * 1e-3) / HBM_ROOF})
        if len(outs) == 2:
            res["cases"][-1]["max_rel_diff_to_two_level"] = float((outs["dense"] - outs["two_level"]).abs().max() / outs["two_level"].abs().max())
        if not args.no_host:
            a = frames[0].cpu().numpy()
            t = []
            for _ in range(2):
                t0 = time.perf_counter()
                rps = np.square(np.abs(np.fft.fftshift(np.fft.rfft2(a), 0))) / norm
                ps = np.empty((L, L))
                ps[:, L // 2:] = rps[:, :-1]
                ps[1:, : L // 2] = rps[L - 1: 0: -1, L // 2: 0: -1]
                ps[0, : L // 2] = rps[0, L // 2: 0: -1]
                np.average(np.reshape(ps, (L // 8, 8, L // 8, 8)), axis=(1, 3))
                t.append((time.perf_counter() - t0) * 1e3)
            res["cases"].append({"L": L, "route": "numpy_host_float32", "ms_per_frame": min(t)})
        del frames
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "noisespec_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
