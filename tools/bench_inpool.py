#!/usr/bin/env python3
"""Times the input side of one exposure of a block (seam 17, pyimcom_amd.inpool) against the path that was available before it, from this
one tool: one 4088 x 4088 TAN-SIP image against a 48 x 48-stamp STG block (n1P = 48, n2 = 32, 0.0390625 arcsec an output pixel), n_inframe = 4.

    fused      inpool.partition_image (the node positions, the relevance loop on the host, one imcom_partition_wcs) and extract_layers
               of layers that are on the device already
    composed   the positions of the visited pixels from wcs._pix2pix (a point list built on the host by select.visiting_order and uploaded),
               select.partition_pixels on them, then InImage.extract_layers' loop as numpy on the downloaded indices and host layers

Both form the same arrays (tests/test_gpu_inpool.py holds them equal at full size).  The median of the timed repetitions after warm-up calls,
by a host clock around work that ends in a device synchronise.  No speed is promised: the file records both times.  Prints one JSON line
and writes it to profiles/inpool_bench.json (or to the path in INPOOL_BENCH_OUT).

    python tools/bench_inpool.py [--reps 5] [--warmup 2]"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NSIDE, N1P, N2, N_INFRAME = 4088, 48, 32, 4
DTHETA = 0.0390625 / 3600.0


def median_ms(fn, torch, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return {"ms": 1e3 * statistics.median(ts), "ms_min": 1e3 * min(ts), "ms_max": 1e3 * max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch

    from pyimcom_amd import _lib, inpool, select
    from pyimcom_amd import wcs as W
    from tests.golden.make_golden_wcs import _header, _rot, _sip

    a = W.DeviceWCS.from_header(_header("TAN-SIP", 53.1, -40.0, _rot(0.11 / 3600.0, 30.0, 1), 2044.5, _sip(4, 3, 3, 2044.0)), array_shape=(NSIDE, NSIDE))
    b = W.DeviceWCS.from_header(_header("STG", 53.1, -40.0, _rot(DTHETA, 0.0, 1), N1P * N2 / 2 + 0.5), array_shape=(N1P * N2, N1P * N2))
    nst = N1P + 2
    use = np.ones((nst, nst), dtype=bool)
    rng = np.random.default_rng(3)
    mask = rng.uniform(size=(NSIDE, NSIDE)) > 0.02
    indata = rng.standard_normal((N_INFRAME, NSIDE, NSIDE)).astype(np.float32)
    indata_d = torch.as_tensor(indata, device="cuda:0")
    mask_d = torch.as_tensor(mask.view(np.uint8), device="cuda:0")
    npixmax = inpool.npixmax_of(N2, DTHETA)
    res = {"tool": "bench_inpool", "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "source_sha16": _lib.source_sha16(),
           "nside": NSIDE, "n1P": N1P, "n2": N2, "n_inframe": N_INFRAME, "npixmax": npixmax}

    def fused():
        part = inpool.partition_image(a, b, use, N2, N1P, npixmax, mask=mask_d)
        return part, part.extract_layers(indata_d)

    def composed():
        is_relevant, matrix, sp_arr = inpool.relevant_cells(a, b, use, N2, N1P, nside=NSIDE)
        vy, vx = select.visiting_order(matrix, sp_arr)
        ox, oy, _, _ = W._pix2pix(a, b, points=np.stack((vx, vy), axis=1).astype(np.float64), nside=NSIDE, want="x")
        y_idx, x_idx, y_val, x_val, count = select.partition_pixels(ox, oy, vx, vy, mask[vy, vx], use, N2, N1P, npixmax)
        yi, xi, cnt = y_idx.cpu().numpy(), x_idx.cpu().numpy(), count.cpu().numpy()
        data = np.zeros((N_INFRAME, nst, nst, int(cnt.max())), dtype=np.float32)
        for j in range(nst):  # coadd.py:399-404
            for i in range(nst):
                n = cnt[j, i]
                data[:, j, i, :n] = indata[:, yi[j, i, :n], xi[j, i, :n]]
        return (y_idx, x_idx, y_val, x_val, count), data

    part, data = fused()
    ref, data_ref = composed()
    same = all(torch.equal(g.view(torch.uint8), w.view(torch.uint8)) for g, w in zip((part.y_idx, part.x_idx, part.y_val, part.x_val, part.pix_count), ref))
    res["equal"] = bool(same and np.array_equal(data.cpu().numpy(), data_ref))
    res["visited"], res["kept"], res["max_count"], res["relevant_cells"] = part.n_visited, int(part.pix_count_host.sum()), part.max_count, int(part.relevant_matrix.sum())
    res["fused"] = median_ms(fused, torch, args.reps, args.warmup)
    res["composed"] = median_ms(composed, torch, args.reps, args.warmup)
    res["composed"]["what"] = "relevant_cells, select.visiting_order, wcs._pix2pix of the uploaded point list, select.partition_pixels, numpy extract_layers"
    line = json.dumps(res)
    print(line)
    out = os.environ.get("INPOOL_BENCH_OUT") or os.path.join(ROOT, "profiles", "inpool_bench.json")
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
