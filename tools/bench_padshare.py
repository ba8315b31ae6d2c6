#!/usr/bin/env python3
"""Times the sharing of padding stamps between device-resident blocks (pyimcom_amd.padshare, csrc/block.hip, seam 20) at the production
shape that tools/bench_metamosaic.py uses: n1 = 84, n2 = 32, postage_pad = 2 (blocks of 2816 x 2816), fade_kernel = 3, six float32 layers,
twelve exposures, all five quality maps:

    pair      one ``update`` (right, adding): three launches
    share     ``share_padding_stamps`` over a resident 3 x 3 grid: twelve pairs of neighbours, 24 updates
    copy      a device-to-device ``copy_`` of a float32 tensor of a block's PRIMARY size; the strips' rate -- the bytes they move (PRIMARY:
              two reads and a write of the strip per plane; INWEIGHT: a read and a write per common exposure; maps: two code reads and a
              code write) over the time -- is reported as a fraction of this copy's rate, counted the same way (bytes read + written)
    numpy     tests/padshare_reference.py's restatement of the same pair update on the host this runs on, and whether the two agree
              (PRIMARY and INWEIGHT bit for bit, the codes within one count: numpy's float32 log10 is not correctly rounded)

Device time by events around the calls (the median of the repetitions after warm-up calls) and the kernels' own time from the library's
event scopes.  The timing is no gate.  Prints one JSON line and writes it to profiles/padshare_bench.json (or to the path in
PADSHARE_BENCH_OUT).

    python tools/bench_padshare.py [--reps 7] [--warmup 2] [--small]"""

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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="n1P = 8, n2 = 4: a rehearsal of the tool, not a measurement")
    args = ap.parse_args()
    import torch

    from pyimcom_amd import _lib
    from pyimcom_amd import padshare as P
    from tests import padshare_reference as PR

    n1P, n2, pad, fk, nlayer, nexp, n_out = (8, 4, 2, 2, 3, 4, 1) if args.small else (88, 32, 2, 3, 6, 12, 1)
    N, width = n1P * n2, pad * n2
    dev = torch.device("cuda:0")
    ctx = _lib.default_context(0)
    name, prop = torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0)
    arch = str(getattr(prop, "gcnArchName", "")).split(":")[0]
    res = {"tool": "bench_padshare", "reps": args.reps, "warmup": args.warmup, "device": name, "arch": arch, "compute_units": int(prop.multi_processor_count),
           "measured_on_mi355x": "MI355X" in name or (arch == "gfx950" and int(prop.multi_processor_count) == 256), "source_sha16": _lib.source_sha16(),
           "n1P": n1P, "n2": n2, "postage_pad": pad, "fade_kernel": fk, "nlayer": nlayer, "n_exposures": nexp, "n_out": n_out, "block_side": N, "small": bool(args.small)}

    gen = torch.Generator(device=dev).manual_seed(20)
    idscas = [(100 + k, 1 + k % 18) for k in range(nexp)]

    def block():
        maps = {}
        for hdu, (letter, coef, dtype, unit, comment) in PR.MAPS.items():
            lo, hi = PR.code_range(dtype)
            codes = torch.randint(lo, hi + 1, (n_out, N, N), generator=gen, device=dev, dtype=torch.int32).to(torch.int16)  # (wraps: all bit patterns)
            maps[hdu] = (codes.view(torch.uint16) if lo == 0 else codes, unit, comment)
        return P.ShareBlock(torch.randn((n_out, nlayer, N, N), generator=gen, device=dev), torch.rand((n_out, nexp, n1P, n1P), generator=gen, device=dev), idscas, maps,
                            n2, pad, fk)

    grid = [[block() for _ in range(3)] for _ in range(3)]
    strip = (width + fk) * N
    res["pair_bytes"] = n_out * (nlayer * strip * 12 + nexp * pad * n1P * 8 + len(PR.MAPS) * strip * 6)
    res["share_bytes"] = 24 * res["pair_bytes"]

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ctx.profile_enable(True)
        ctx.profile_reset()
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        ms_k, launches = ctx.profile_get("padshare")
        ctx.profile_enable(False)
        return {"ms": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts), "ms_kernels": ms_k / args.reps, "launches_per_call": launches / args.reps}

    mine_h = {k: v.cpu().numpy() for k, v in (("primary", grid[0][0].primary), ("inweight", grid[0][0].inweight))}
    mine_h["maps"] = {k: v[0].cpu().numpy() for k, v in grid[0][0].maps.items()}
    res["pair"] = timed(lambda: P.update(grid[0][0], grid[0][1], "right", True))
    res["share"] = timed(lambda: P.share_padding_stamps(3, grid))
    a, b = torch.empty((n_out, nlayer, N, N), dtype=torch.float32, device=dev), torch.zeros((n_out, nlayer, N, N), dtype=torch.float32, device=dev)
    res["copy"] = timed(lambda: a.copy_(b))
    res["copy_bytes"] = 2 * 4 * a.numel()
    res["copy_GBps"] = res["copy_bytes"] / (1e-3 * res["copy"]["ms"]) / 1e9
    for what in ("pair", "share"):
        for key in ("ms", "ms_kernels"):
            rate = res[what + "_bytes"] / (1e-3 * res[what][key]) / 1e9
            res[f"{what}_GBps" + ("" if key == "ms" else "_kernels")] = rate
            res[f"{what}_fraction_of_copy_rate" + ("" if key == "ms" else "_kernels")] = rate / res["copy_GBps"]

    # the numpy restatement of one pair update on this host, from the first block's state before any update and an untouched neighbour
    fresh = block()
    theirs_h = {"primary": fresh.primary.cpu().numpy(), "inweight": fresh.inweight.cpu().numpy(), "idscas": idscas,
                "maps": {k: [v[0].cpu().numpy(), v[1], v[2]] for k, v in fresh.maps.items()}}
    host_mine = {"primary": mine_h["primary"], "inweight": mine_h["inweight"], "idscas": idscas,
                 "maps": {k: [mine_h["maps"][k], v[1], v[2]] for k, v in fresh.maps.items()}}
    dev_mine = P.ShareBlock.from_arrays(host_mine["primary"], host_mine["inweight"], idscas, {k: tuple(v) for k, v in host_mine["maps"].items()}, n2, pad, fk)
    P.update(dev_mine, fresh, "right", True)
    t0 = time.perf_counter()
    PR.update(host_mine, theirs_h, "right", True, n2, pad, fk)
    t_host = time.perf_counter() - t0
    got = dev_mine.to_arrays()
    apart = {k: np.abs(got["maps"][k][0].astype(np.int64) - host_mine["maps"][k][0].astype(np.int64)) for k in got["maps"]}
    res["numpy"] = {"pair_s": t_host, "host_cpus": os.cpu_count(), "primary_equals_device": PR.same_bits(got["primary"], host_mine["primary"]),
                    "inweight_equals_device": PR.same_bits(got["inweight"], host_mine["inweight"]), "codes_largest_difference": int(max(d.max() for d in apart.values())),
                    "codes_differing_share_of_strip": float(sum(int((d != 0).sum()) for d in apart.values()) / (len(apart) * n_out * strip))}
    res["numpy_pair_over_device"] = t_host / (1e-3 * res["pair"]["ms"])
    line = json.dumps(res)
    print(line)
    out = os.environ.get("PADSHARE_BENCH_OUT", os.path.join(ROOT, "profiles", "padshare_bench.json"))
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
