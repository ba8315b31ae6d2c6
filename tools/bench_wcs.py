#!/usr/bin/env python3
"""Times the device WCS of pyimcom_amd.wcs (csrc/wcs.hip) at the size the reference runs it, 4088 x 4088 pixels of one SCA:

    map           map_sca2sca, TAN-SIP -> TAN-SIP, float64 positions with mask and count, everything left on the device
    map_tables    the same with float32 error tables on both sides and niter = 3 ("ASTROPY+")
    pix2world     all_pix2world of the 4088^2 pixel list, list and result on the device
    count_only    the count-only map at subsamp = 8 (one pair of get_overlap_matrix)

The median of the timed repetitions after warm-up calls, by a host clock around work that ends in a device synchronise, and the kernels' own
time from the library's event scopes.  Next to each the bytes the launch writes and reads (counted, not measured: the plain map writes 17
bytes a pixel and reads nothing, so the store rate is its roof) and their share of the 6.3 TB/s copy rate of this chip over the kernels'
time.  The numpy restatement of the same chain (tests/wcs_reference.py) is timed on a stated fraction of the pixels on the host this runs
on and scaled: the yardstick to quote beside the device's figures.  The reference's own astropy time cannot be measured where astropy is
not installed.  Prints one JSON line and writes it to profiles/wcs_bench.json (or to the path in WCS_BENCH_OUT).

    python tools/bench_wcs.py [--reps 7] [--warmup 2] [--host-fraction 0.02]"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NSIDE = 4088
COPY_RATE = 6.3e12  # bytes / s, the measured copy rate of the chip


def timed(fn, ctx, torch, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ctx.profile_enable(True)
    ctx.profile_reset()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ms_k, launches = ctx.profile_get("wcs")
    ctx.profile_enable(False)
    return {"ms": 1e3 * statistics.median(ts), "ms_min": 1e3 * min(ts), "ms_max": 1e3 * max(ts), "ms_kernels": ms_k / reps, "launches_per_call": launches / reps}


def traffic(res, written, read):
    res["bytes_written"], res["bytes_read"] = int(written), int(read)
    res["share_of_copy_rate_over_kernels"] = (written + read) / (res["ms_kernels"] * 1e-3) / COPY_RATE if res["ms_kernels"] > 0 else None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-fraction", type=float, default=0.02)
    args = ap.parse_args()
    import torch

    from pyimcom_amd import _lib
    from pyimcom_amd import wcs as W
    from tests import wcs_reference as R

    G = np.load(os.path.join(ROOT, "tests", "golden", "wcs.npz"))
    meta = {c["name"]: c for c in json.loads(str(G["meta"]))["cases"]}
    ctx = _lib.default_context(0)
    res = {"tool": "bench_wcs", "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "source_sha16": _lib.source_sha16(),
           "nside": NSIDE, "copy_rate_bytes_per_s": COPY_RATE, "astropy": "not installed where this ran: the reference's own time is not measured"}
    a = W.DeviceWCS.from_header(meta["sip2_m40"]["header"])
    b = W.DeviceWCS.from_header(meta["sip2_m40_b"]["header"])
    n = NSIDE * NSIDE
    # error tables at the reference's size: a smooth float32 map of 4088^2 nodes, padded as err_interp pads it
    yy, xx = np.mgrid[0:NSIDE, 0:NSIDE].astype(np.float32) / NSIDE
    raw = np.stack((0.05 * np.sin(3 * xx + yy), 0.04 * np.cos(2 * yy - xx))).astype(np.float32)
    tab = W.error_table(raw, a=8, n_pad=NSIDE // 2, use_float32=True)
    del yy, xx, raw
    at = W.DeviceWCS.from_header(meta["sip2_m40"]["header"], table=tab, niter=3)
    bt = W.DeviceWCS.from_header(meta["sip2_m40_b"]["header"], table=tab, niter=3)
    grid = [0.0, 1.0, NSIDE, 0.0, 1.0, NSIDE]

    res["map"] = traffic(timed(lambda: W._pix2pix(a, b, grid=grid, nside=NSIDE), ctx, torch, args.reps, args.warmup), 17 * n, 0)
    # four taps of two planes a look-up; one look-up forward, niter in the inverse; neighbouring pixels share cache lines, so this is an upper count
    res["map_tables"] = traffic(timed(lambda: W._pix2pix(at, bt, grid=grid, nside=NSIDE), ctx, torch, args.reps, args.warmup), 17 * n, (1 + 3) * 8 * 4 * n)
    res["map_tables"]["note"] = "bytes_read counts every tap of every look-up (float32, 8 taps, 1 + niter look-ups a pixel) as if none hit a cache"
    s = torch.arange(NSIDE, dtype=torch.float64, device="cuda")
    pts = torch.stack((s.repeat(NSIDE), s.repeat_interleave(NSIDE)), 1).contiguous()
    res["pix2world"] = traffic(timed(lambda: a.all_pix2world(pts, 0), ctx, torch, args.reps, args.warmup), 16 * n, 16 * n)
    lo, step, cnt = W._grid_axis(NSIDE, 0, 8)
    res["count_only"] = traffic(timed(lambda: W._pix2pix(a, b, grid=[lo, step, cnt, lo, step, cnt], nside=NSIDE, want=""), ctx, torch, args.reps, args.warmup), 16, 0)
    res["count_only"]["points"] = cnt * cnt
    _, _, _, counts = W._pix2pix(a, b, grid=grid, nside=NSIDE)
    res["map"]["in_ref"], res["map"]["nan"] = counts

    # the host's restatement on a fraction of the rows
    rows = max(1, int(round(args.host_fraction * NSIDE)))
    xi, yi = np.meshgrid(np.arange(NSIDE, dtype=np.float64), np.arange(rows, dtype=np.float64))
    t0 = time.perf_counter()
    R.np_pix2pix(a.descriptor, None, b.descriptor, None, xi, yi, 0)
    t1 = time.perf_counter()
    R.np_pix2world(a.descriptor, None, xi, yi, 0)
    t2 = time.perf_counter()
    res["host"] = {"what": "numpy restatement (tests/wcs_reference.py) on the first rows of the grid, scaled to 4088 rows", "rows": rows, "cpus": os.cpu_count(),
                   "map_s_scaled": (t1 - t0) * NSIDE / rows, "pix2world_s_scaled": (t2 - t1) * NSIDE / rows}
    line = json.dumps(res)
    print(line)
    out = os.environ.get("WCS_BENCH_OUT") or os.path.join(ROOT, "profiles", "wcs_bench.json")
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
