#!/usr/bin/env python3
"""Time the input-layer cube on the device (pyimcom_amd.layers.build_cube; INTEGRATION.md seam 23).  One production cube of nside^2 pixels,
extrainput = ["", "cstar14", "nstar14,2e5,86,3", "whitenoise10", "1fnoise9", "labnoise"], from a big-endian float32 science frame with a
sky value, a 4096^2 big-endian labnoise file and a synthetic float64 star image on the device, built and left on the device.  In the same
run the route it replaces: the per-seam calls of INTEGRATION.md seams 5 / 13 / 22 with their host round trips (the star image downloaded,
the nstar, white-noise and 1/f frames handed back as numpy), numpy's subtraction, cast and byte swap of the file planes on the host this
runs on, and the upload of the finished cube.  Also imcom_layer_place alone on a nside^2 big-endian float32 plane already on the device:
bytes moved (4 read + 4 written a pixel) over its event time, against the HBM rates of the MI355X (8.0 TB/s specified, 6.29 TB/s measured
for a float4 copy).  One JSON line, also written to profiles/layercube_bench.json.

    python tools/bench_layercube.py [--nside 4088] [--reps 3] [--warmup 1]
"""

import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nside", type=int, default=4088)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import torch

    from pyimcom_amd import _lib, inject, layers, noiselayers as nl
    from pyimcom_amd._dev import bound_context

    n, idsca, dev, sky = args.nside, (4321, 7), "cuda:0", 86.123456789
    if n != 4088:
        raise SystemExit("the 1/f layer is a [4088, 4088] frame: --nside 4088")
    names = ["", "cstar14", "nstar14,2e5,86,3", "whitenoise10", "1fnoise9", "labnoise"]
    rng = np.random.default_rng(23)
    sci = (sky + 12.0 * rng.standard_normal((n, n), dtype=np.float32)).astype(">f4")
    lab = (3.0 * rng.standard_normal((n + 8, n + 8), dtype=np.float32)).astype(">f4")
    x = np.arange(n, dtype=np.float64)
    prof = np.exp(-0.5 * ((x[:, None] - np.arange(58.5, n, 117.0)[None, :]) / 1.6) ** 2).sum(axis=1)
    brightness = torch.from_numpy(prof[:, None] * prof[None, :] / (2 * np.pi * 1.6**2) - 2.0e-5).to(dev)
    cfg = types.SimpleNamespace(n_inframe=len(names), extrainput=names, informat="dc2_imsim", inpsf_oversamp=8)
    files = {"sci": (sci, sky), "labnoise": lab}
    res = {"what": "build_cube", "nside": n, "extrainput": names, "cube_bytes": 4 * len(names) * n * n, "device": torch.cuda.get_device_name(0),
           "source": _lib.source_sha16()}

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

    def device_route():
        return layers.build_cube(cfg, idsca, lambda kind, label=None: files.get(kind), grid_image=lambda r: brightness, nside=n)

    def host_route():
        cube = np.zeros((len(names), n, n), dtype=np.float32)
        cube[0] = sci - sky  # layer.py:1261 on the host: byte swap, subtraction, one pass
        cube[1] = brightness.cpu().numpy()  # seam 5: make_image_from_grid ends in .cpu().numpy()
        cube[2] = inject.nstar_layer(brightness.cpu().numpy(), 2.0e5, 86.0, 3, idsca)  # seam 22's snippet (the reference forms the image again)
        cube[3] = nl.white_noise_frame(layers.layer_seed(10, idsca), n)  # seam 13's snippet: float64 on the host
        cube[4] = nl.noise_1f_frame(layers.layer_seed(9, idsca))
        cube[5] = lab[4:4092, 4:4092]  # layer.py:1324
        return torch.from_numpy(cube).to(dev)

    res["ms_device"], res["ms_device_min"] = timed(device_route)
    res["ms_host_route"], res["ms_host_route_min"] = timed(host_route)
    a, b = device_route(), host_route()
    res["equal_to_host_route"] = bool(torch.equal(a, b))
    del a, b

    # the kernel alone: a big-endian float32 plane on the device, minus the sky
    ctx = bound_context(dev)
    raw = torch.from_numpy(sci.view(np.uint8).reshape(-1).copy()).to(dev)
    dst = torch.empty((n, n), dtype=torch.float32, device=dev)
    calls = 20

    def kernel():
        _lib.check(_lib.lib.imcom_layer_place(ctx.handle, _lib.ptr(raw), 0, 1, n, n, 0, 0, 0, 1, sky, 0, 0.0, _lib.ptr(dst), n, _lib.MEM_DEVICE))

    for _ in range(3):
        kernel()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        kernel()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / calls
    tbs = 8.0 * n * n / (ms * 1e-3) / 1e12
    res["layer_place"] = {"plane": "big-endian float32, minus sky", "calls": calls, "ms_event": ms, "bytes": 8 * n * n, "TB_per_s": tbs,
                          "share_of_hbm_spec": tbs / HBM_SPEC_TBS, "share_of_measured_copy": tbs / HBM_COPY_TBS, "bound": "bytes"}
    res["layer_place"]["equal_to_numpy"] = bool(torch.equal(dst, torch.from_numpy(sci - sky).to(dev)))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "layercube_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
