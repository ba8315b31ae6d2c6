#!/usr/bin/env python3
"""Times the device HEALPix star grid of pyimcom_amd.healpix (csrc/wcs.hip) at the size the reference runs it: res = 14 and the radius of one
SCA side (4088 x 0.11 arcsec) about the centre of a TAN-SIP SCA, the cap plus the positions ``x, y`` through the WCS
(``generate_star_grid``):

    grid_device   generate_star_grid(14, wcs, device_out=True): the centre, the count, the allocation and the fill, results left on the device
    grid_host     the same with the five arrays brought to the host (numpy results, what make_image_from_grid takes)
    numpy         the numpy restatement of the reference's statements (tests/healpix_reference.py standing in for healpy, tests/wcs_reference.py
                  for the WCS) on the host this runs on: every pixel between the two declinations is tested, as make_sph_grid does

The median of the timed repetitions after warm-up calls, by a host clock around work that ends in a device synchronise, and the kernels' own
time from the library's event scopes.  The reference's own time with healpy cannot be measured where healpy is not installed.  The timing is
no gate.  Prints one JSON line and writes it to profiles/healpix_bench.json (or to the path in HEALPIX_BENCH_OUT).

    python tools/bench_healpix.py [--reps 9] [--warmup 2] [--host-reps 1]"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RES = 14


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=1)
    args = ap.parse_args()
    import torch

    from pyimcom_amd import _lib
    from pyimcom_amd import healpix as H
    from pyimcom_amd import wcs as W
    from tests import healpix_reference as R
    from tests import wcs_reference as RW

    G = np.load(os.path.join(ROOT, "tests", "golden", "wcs.npz"))
    header = next(c for c in json.loads(str(G["meta"]))["cases"] if c["name"] == "sip2_m40_b")["header"]
    w = W.DeviceWCS.from_header(header)
    ctx = _lib.default_context(0)
    name, prop = torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0)
    arch = str(getattr(prop, "gcnArchName", "")).split(":")[0]
    # (the driver may report a generic name; the architecture and the compute units say what the device is: gfx950 with 256 CUs)
    res = {"tool": "bench_healpix", "reps": args.reps, "warmup": args.warmup, "device": name, "arch": arch, "compute_units": int(prop.multi_processor_count),
           "measured_on_mi355x": "MI355X" in name or (arch == "gfx950" and int(prop.multi_processor_count) == 256),
           "source_sha16": _lib.source_sha16(), "res": RES, "radius_rad": 4088 * 0.11 / 3600 * (np.pi / 180),
           "healpy": "not installed where this ran: the reference's own time is not measured"}

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ctx.profile_enable(True)
        ctx.profile_reset()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ms_k, launches = ctx.profile_get("healpix")
        ms_w, launches_w = ctx.profile_get("wcs")
        ctx.profile_enable(False)
        return out, {"ms": 1e3 * statistics.median(ts), "ms_min": 1e3 * min(ts), "ms_max": 1e3 * max(ts), "ms_kernels": (ms_k + ms_w) / args.reps,
                     "launches_per_call": (launches + launches_w) / args.reps}

    dev, res["grid_device"] = timed(lambda: H.generate_star_grid(RES, w, device_out=True))
    host, res["grid_host"] = timed(lambda: H.generate_star_grid(RES, w))
    res["npix"] = int(host[0].size)
    assert all(torch.is_tensor(t) and t.is_cuda for t in dev) and np.array_equal(dev[0].cpu().numpy(), host[0])

    # the reference's statements, restated: all_pix2world of the centre, every pixel pmin .. pmax through pix2ang and the predicate, all_world2pix
    def restated():
        degree = np.pi / 180
        cen = RW.np_pix2world(w.descriptor, None, np.array([2043.5]), np.array([2043.5]), 0)
        ra, dec, radius = float(cen[0][0]) * degree, float(cen[1][0]) * degree, res["radius_rad"]
        pmin, pmax = R.reference_range(1 << RES, ra, dec, radius)
        ipix, theta, phi, _ = R.cap_brute(1 << RES, ra, dec, radius, pmin, pmax, chunk=1 << 30)
        x, y, _ = RW.np_world2pix(w.descriptor, None, phi / degree, (np.pi / 2.0 - theta) / degree, 0)
        return ipix, x, y, pmax - pmin + 1

    ts = []
    for _ in range(max(1, args.host_reps)):
        t0 = time.perf_counter()
        ipix, x, y, candidates = restated()
        ts.append(time.perf_counter() - t0)
    assert np.array_equal(ipix, host[0])
    res["numpy"] = {"s": statistics.median(ts), "candidates": int(candidates), "kept": int(ipix.size), "host_cpus": os.cpu_count(),
                    "largest_difference_from_device_pixel": float(max(np.max(np.abs(x - host[1])), np.max(np.abs(y - host[2]))))}
    res["numpy_over_grid_host"] = res["numpy"]["s"] / (1e-3 * res["grid_host"]["ms"])
    line = json.dumps(res)
    print(line)
    out = os.environ.get("HEALPIX_BENCH_OUT", os.path.join(ROOT, "profiles", "healpix_bench.json"))
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
