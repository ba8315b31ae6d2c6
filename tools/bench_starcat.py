#!/usr/bin/env python3
"""Times the star catalog of pyimcom_amd.starcat on the device: ``star_moments`` (the adaptive moments, the fourth moments and the
forced-scale moments of csrc/starmom.hip, one launch) for one block's worth of stars -- a 2688 x 2688 float32 frame, 400 stars, bd = 40 --
and for 16 such blocks, the frames already on the device and the results left there; then the whole ``star_catalog`` row of one block
(numpy maps uploaded, table read back).  The median of the timed repetitions after warm-up calls, by a host clock around work that ends in
a device synchronise, and the kernels' own time from the library's event scopes.  Next to each what the launch does, counted and not
measured: the iterations per star (read back from the result), the pixels under the weight ellipse summed over the iterations (counted by
the numpy restatement of tests/starcat_reference.py on a stated fraction of the stars and scaled), the ``exp`` calls and float64
operations that follow from them (an ``exp`` counted as one operation, so the share understates the work), the bytes read and written, and
the share of the 78.6 TF/s float64 vector peak of DESIGN.md over the kernels' time.  The same fraction of the stars is timed through the
restatement on the host this runs on: the yardstick to quote beside the device's figures (the reference itself needs GalSim).  Prints one
JSON line and writes it to profiles/starcat_bench.json (or to the path in STARCAT_BENCH_OUT).

    python tools/bench_starcat.py [--reps 7] [--warmup 2] [--host-fraction 0.1]"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIDE, NSTAR, BD, BD2, N2, FORCED_SCALE = 2688, 400, 40, 8, 48, 0.40 / 0.0390625
FP64_VECTOR_PEAK = 78.6e12  # flop / s
# float64 operations a pixel: the weighted sums of an iteration (rho2 5 mul + 2 add, exp, 1 + 2 + 3 + 2 mul, 7 add) and the two last passes
# (u, v: 4 mul 2 sub 2 div; squares and the weight: 4 mul 1 add 1 mul exp 1 mul; the terms: 9 mul 3 add 3 add; forced: 2 mul 1 add 1 mul 1 div exp 1 mul, 4 mul 1 sub, 3 add)
OPS_ITER_PIXEL, OPS_LAST_PIXEL, EXP_LAST_PIXEL = 23, 45, 2


def block(seed):
    """A frame with NSTAR stars on a 20 x 20 grid, each with its own flux, width, shape and sub-pixel position."""
    from tests import starcat_reference as R

    rng = np.random.default_rng(seed)
    pitch = (SIDE - 2 * 100) / 19.0
    gx, gy = np.meshgrid(100 + pitch * np.arange(20), 100 + pitch * np.arange(20))
    x = gx.ravel() + rng.uniform(-0.5, 0.5, NSTAR)
    y = gy.ravel() + rng.uniform(-0.5, 0.5, NSTAR)
    frame = np.zeros((SIDE, SIDE), dtype=np.float32)
    for k in range(NSTAR):
        cx, cy = int(np.rint(x[k])), int(np.rint(y[k]))
        e1, e2 = rng.uniform(-0.1, 0.1, 2)
        frame[cy - 20:cy + 21, cx - 20:cx + 21] = R.draw_star(41, x[k] - cx + 20, y[k] - cy + 20, rng.uniform(1, 5), rng.uniform(2.2, 2.8), e1, e2, 0.1)
    return frame, x, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-fraction", type=float, default=0.1)
    args = ap.parse_args()
    import torch

    from pyimcom_amd import _lib, starcat
    from tests import starcat_reference as R

    ctx = _lib.default_context(0)
    res = {"tool": "bench_starcat", "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "source_sha16": _lib.source_sha16(), "side": SIDE,
           "stars_per_block": NSTAR, "bd": BD, "forced_scale": FORCED_SCALE, "fp64_vector_peak_flop_per_s": FP64_VECTOR_PEAK}
    frame, x, y = block(1)
    # the host's restatement on a fraction of the stars: its time, and the pixels under the ellipse an iteration
    nhost = max(1, int(round(args.host_fraction * NSTAR)))
    xi, yi = np.rint(x).astype(int), np.rint(y).astype(int)
    pixels = 0
    t0 = time.perf_counter()
    for k in range(nhost):
        cut = frame[yi[k] + 1 - BD:yi[k] + BD, xi[k] + 1 - BD:xi[k] + BD]  # (analysis.py:1001)
        trace = []
        m = R.find_adaptive_mom(cut, trace=trace)
        R.higher_moments(cut, m, FORCED_SCALE)
        pixels += sum(int(np.sum(t[3] - t[2] + 1)) for t in trace)
    host_s = time.perf_counter() - t0
    res["host"] = {"what": "numpy restatement (tests/starcat_reference.py): moments and the two last passes", "stars": nhost, "fraction": nhost / NSTAR, "s": host_s,
                   "s_per_block_scaled": host_s * NSTAR / nhost, "cpus": os.cpu_count()}
    side = 2 * BD - 1
    for blocks in (1, 16):
        frames = torch.as_tensor(np.stack([frame] * blocks)).to("cuda:0")
        wall, kern, tab = [], [], None
        for i in range(args.warmup + args.reps):
            ctx.profile_enable(True)
            ctx.profile_reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b in range(blocks):
                tab = starcat.star_moments(frames[b], x, y, BD, FORCED_SCALE)["table"]
            torch.cuda.synchronize()
            if i >= args.warmup:
                wall.append((time.perf_counter() - t0) * 1e3)
                kern.append(ctx.profile_get("star_moments")[0])
            ctx.profile_enable(False)
        t = tab.cpu().numpy()
        iters, ok = t[:, starcat._NITER], t[:, starcat._STATUS] == 0
        sum_pixels = pixels * NSTAR / nhost  # pixel visits of the iterations, one launch (scaled from the host's fraction)
        last = int(ok.sum()) * side * side
        ops = blocks * (sum_pixels * OPS_ITER_PIXEL + last * OPS_LAST_PIXEL)
        k = statistics.median(kern)
        res[f"blocks_{blocks}"] = {"ms": statistics.median(wall), "ms_min": min(wall), "ms_max": max(wall), "ms_kernels": k, "stars_per_s": blocks * NSTAR / statistics.median(wall) * 1e3,
                                   "converged": int(ok.sum()), "iterations_per_star": {"mean": float(iters.mean()), "min": int(iters.min()), "max": int(iters.max())},
                                   "per_launch": {"bytes_read": NSTAR * side * side * 4 + NSTAR * 8, "bytes_written": NSTAR * starcat.NCOL * 8,
                                                  "exp_calls": sum_pixels + last * EXP_LAST_PIXEL, "float64_ops": ops / blocks},
                                   "share_of_fp64_vector_peak_over_kernels": ops / FP64_VECTOR_PEAK / (k * 1e-3) if k > 0 else None}
    # the whole catalog row of one block: numpy maps in, the table out
    rng = np.random.default_rng(2)
    maps = {"fidelity": (rng.integers(15000, 30000, (SIDE, SIDE)).astype(np.uint16), 0.0002), "inweight": rng.random((6, SIDE // N2, SIDE // N2)).astype(np.float32),
            "uc": rng.random((SIDE, SIDE)).astype(np.float32), "sigma": rng.random((SIDE, SIDE)).astype(np.float32), "tsum": rng.random((SIDE, SIDE)).astype(np.float32),
            "neff": rng.random((SIDE, SIDE)).astype(np.float32)}
    wall = []
    for i in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cat = starcat.star_catalog(frame, x, y, bd=BD, bd2=BD2, forced_scale=FORCED_SCALE, n2=N2, **maps)
        torch.cuda.synchronize()
        if i >= args.warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    res["catalog_one_block_numpy_in_out"] = {"ms": statistics.median(wall), "ms_min": min(wall), "ms_max": max(wall), "rows": int(cat.shape[0]),
                                             "note": "six 2688 x 2688 maps uploaded per call: the copies, not the kernels"}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    out = os.environ.get("STARCAT_BENCH_OUT") or os.path.join(ROOT, "profiles", "starcat_bench.json")
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
