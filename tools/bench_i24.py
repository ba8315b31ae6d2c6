#!/usr/bin/env python3
"""Times the I24 layer codec of pyimcom_amd.i24 on the device: ``compress_layers`` and ``decompress_layers`` of 2688 x 2688 float32
layers, 1 and 16 in a batch, with the documented parameters (BITKEEP 20, DIFF, SOFTBIAS -1, I24B with REORDER), the layers already on the
device and the results left there; the median of the timed repetitions after warm-up calls, by a host clock around work that ends in a
device synchronise (compress reads the overflow counts back between its launches and allocates its outputs, so the host's share is part
of the figure), and the kernels' own time from the library's event scopes.  Next to each the bytes the direction moves per pixel -- counted
from the kernels, not measured -- and what share of the 8 TB/s HBM roof of DESIGN.md that is over the kernels' time.  With
``--reference`` the same layer through the numpy restatement of tests/i24_reference.py on the host this runs on (or through
pyimcom.compress.i24 itself where pyimcom and astropy are installed; the line says which): the yardstick to quote beside the device's
figures.  Prints one JSON line and writes it to profiles/i24_bench.json.

    python tools/bench_i24.py [--reps 7] [--warmup 2] [--reference]"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIDE = 2688
PARS = {"VMIN": -0.5, "VMAX": 1.5, "BITKEEP": 20, "DIFF": True, "SOFTBIAS": -1}
HBM_ROOF = 8.0e12  # bytes / s
# bytes per pixel with nb = 3 byte planes: quantise reads 4 (float32) and writes 4 (code); pack reads 4 and writes 3; the overflow write
# reads only the tiles that hold a hit.  unpack reads 3 and writes 4; the prefix sum + dequantise reads 4 and writes 4.
BYTES_COMPRESS, BYTES_DECOMPRESS = 4 + 4 + 4 + 3, 3 + 4 + 4 + 4


def layers(count, seed=1):
    rng = np.random.default_rng(seed)
    return rng.normal(0.5, 0.4, (count, SIDE, SIDE)).astype(np.float32)  # about 1 pixel in 80 outside VMIN .. VMAX


def host_codec():
    try:
        from pyimcom.compress.i24 import i24compress, i24decompress

        return (lambda im: i24compress(im, "I24B", PARS)), (lambda d, ov: i24decompress(d, "I24B", PARS, overflow=ov)), "pyimcom.compress.i24"
    except ImportError:
        from tests import i24_reference as R

        return (lambda im: R.compress(im, "I24B", PARS)), (lambda d, ov: R.decompress(d, "I24B", PARS, ov)), "numpy restatement (tests/i24_reference.py)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reference", action="store_true")
    args = ap.parse_args()
    import torch

    from pyimcom_amd import _lib, i24

    ctx = _lib.default_context(0)
    res = {"tool": "bench_i24", "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "source_sha16": _lib.source_sha16(), "side": SIDE,
           "pars": PARS, "scheme": "I24B", "bytes_per_pixel": {"compress": BYTES_COMPRESS, "decompress": BYTES_DECOMPRESS}, "hbm_roof_bytes_per_s": HBM_ROOF}
    for count in (1, 16):
        t = torch.as_tensor(layers(count), device="cuda:0")
        pars = [PARS] * count
        out = {}
        cubes = ovs = stacked = back = None
        for name, family, bpp in (("compress", "i24_compress", BYTES_COMPRESS), ("decompress", "i24_decompress", BYTES_DECOMPRESS)):
            wall, kern = [], []
            for i in range(args.warmup + args.reps):
                ctx.profile_enable(True)
                ctx.profile_reset()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if name == "compress":
                    cubes, ovs = i24.compress_layers(t, pars)
                else:
                    back = i24.decompress_layers(stacked, pars, ovs)
                torch.cuda.synchronize()
                if i >= args.warmup:
                    wall.append((time.perf_counter() - t0) * 1e3)
                    kern.append(ctx.profile_get(family)[0])
                ctx.profile_enable(False)
            if name == "compress":
                stacked = torch.stack(cubes)  # one [L, nb, ny, nx] tensor, as a block read from disk arrives: read in place
            npx = count * SIDE * SIDE
            k = statistics.median(kern)
            out[name] = {"ms": statistics.median(wall), "ms_min": min(wall), "ms_max": max(wall), "ms_kernels": k, "gpixel_per_s": npx / statistics.median(wall) / 1e6,
                         "hbm_share_of_kernels": (npx * bpp / HBM_ROOF) / (k * 1e-3) if k > 0 else None}
        out["overflow_entries"] = int(sum(len(o) for o in ovs))
        out["round_trip_max_error"] = float((back - t).abs().max().item())
        res[f"layers_{count}"] = out
    if args.reference:
        comp, decomp, which = host_codec()
        im = layers(1)[0]
        t0 = time.perf_counter()
        d, ov = comp(im)
        t1 = time.perf_counter()
        decomp(d, ov)
        t2 = time.perf_counter()
        res["host"] = {"codec": which, "s_compress_one_layer": t1 - t0, "s_decompress_one_layer": t2 - t1, "cpus": os.cpu_count()}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "i24_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
