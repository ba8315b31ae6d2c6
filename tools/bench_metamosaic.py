#!/usr/bin/env python3
"""Times the device metadetection mosaic of pyimcom_amd.metamosaic (csrc/ginterp.hip, seam 19) at the production shape: n1 = 84, n2 = 32,
postage_pad = 2 (block files of 2816 x 2816, a mosaic of 8064 x 8064), six float32 layers:

    paste     the nine add_block calls of an interior block from device tensors (one launch each); its rate on the bytes the windows
              need (layers read and written, codes read, two dB maps and the mask written) as a fraction of the rate of a device-to-device
              copy_ of a float32 tensor of the mosaic's size, counted the same way (bytes read + bytes written)
    cuts      mask_fidelity_cut + mask_noise_cut
    caps      mask_caps_pixels for 3000 objects of 50 to 500 pixels radius: pixels tested (the pixels of all boxes) per second
    numpy     tests/metamosaic_reference.py's restatement of the same paste and of the circles of the first --host-objects objects on the
              host this runs on

The median of the timed repetitions after warm-up calls, by a host clock around work that ends in a device synchronise, and the kernels' own
time from the library's event scopes.  The timing is no gate.  Prints one JSON line and writes it to profiles/metamosaic_bench.json (or to
the path in METAMOSAIC_BENCH_OUT).

    python tools/bench_metamosaic.py [--reps 7] [--warmup 2] [--host-objects 100] [--small]"""

import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-objects", type=int, default=100)
    ap.add_argument("--small", action="store_true", help="n1 = 4, n2 = 8, pad = 1 and 30 objects: a rehearsal of the tool, not a measurement")
    args = ap.parse_args()
    import torch

    from pyimcom_amd import _lib
    from pyimcom_amd import metamosaic as M
    from tests import metamosaic_reference as MR

    n1, n2, pad, nlayer, nobj, rlo, rhi = (4, 8, 1, 6, 30, 2.0, 20.0) if args.small else (84, 32, 2, 6, 3000, 50.0, 500.0)
    cfgd = {"n1": n1, "n2": n2, "postage_pad": pad, "nblock": 8, "dtheta": 0.04 / 3600.0, "ra": 53.0, "dec": -40.0, "lonpole": 180.0, "outpsf": "GAUSSIAN",
            "sigmatarget": 1.5 / 2.355, "extrainput": [None] * nlayer}
    side = (n1 + 2 * pad) * n2
    dev = torch.device("cuda:0")
    ctx = _lib.default_context(0)
    name, prop = torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0)
    arch = str(getattr(prop, "gcnArchName", "")).split(":")[0]
    res = {"tool": "bench_metamosaic", "reps": args.reps, "warmup": args.warmup, "device": name, "arch": arch, "compute_units": int(prop.multi_processor_count),
           "measured_on_mi355x": "MI355X" in name or (arch == "gfx950" and int(prop.multi_processor_count) == 256), "source_sha16": _lib.source_sha16(),
           "n1": n1, "n2": n2, "postage_pad": pad, "nlayer": nlayer, "block_side": side, "small": bool(args.small)}

    gen = torch.Generator(device=dev).manual_seed(19)
    primary = torch.randn((nlayer, side, side), generator=gen, device=dev, dtype=torch.float32)
    fid = torch.randint(0, 30000, (side, side), generator=gen, device=dev, dtype=torch.int32).to(torch.int16).view(torch.uint16)
    sig = torch.randint(-3000, 3000, (side, side), generator=gen, device=dev, dtype=torch.int32).to(torch.int16)
    m = M.DeviceMetaMosaic(types.SimpleNamespace(**cfgd), 3, 4, nlayer, np.float32)
    ns = m.Nside
    res["Nside"] = ns
    pixels = sum((w[5] - w[4]) * (w[7] - w[6]) for w in m.windows)
    res["paste_bytes"] = pixels * (2 * 4 * nlayer + 2 + 2 + 4 + 4 + 1)

    def timed(fn, family="mosaic"):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ctx.profile_enable(True)
        ctx.profile_reset()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ms_k, launches = ctx.profile_get(family)
        ctx.profile_enable(False)
        return {"ms": 1e3 * statistics.median(ts), "ms_min": 1e3 * min(ts), "ms_max": 1e3 * max(ts), "ms_kernels": ms_k / args.reps, "launches_per_call": launches / args.reps}

    def paste():
        for w in m.windows:
            m.add_block(w[0], w[1], primary, fid, sig, -2e-4, 2e-4)

    res["paste"] = timed(paste)
    a, b = torch.empty((ns, ns), dtype=torch.float32, device=dev), torch.zeros((ns, ns), dtype=torch.float32, device=dev)
    res["copy"] = timed(lambda: a.copy_(b))
    res["copy_bytes"] = 2 * 4 * ns * ns
    res["copy_GBps"] = res["copy_bytes"] / (1e-3 * res["copy"]["ms"]) / 1e9
    for key in ("ms", "ms_kernels"):
        rate = res["paste_bytes"] / (1e-3 * res["paste"][key]) / 1e9
        res["paste_GBps" + ("" if key == "ms" else "_kernels")] = rate
        res["paste_fraction_of_copy_rate" + ("" if key == "ms" else "_kernels")] = rate / res["copy_GBps"]

    def cuts():
        m.mask_fidelity_cut(40.0)
        m.mask_noise_cut(3.0)

    res["cuts"] = timed(cuts)

    rng = np.random.default_rng(19)
    x, y, r = rng.uniform(0.0, ns, nobj), rng.uniform(0.0, ns, nobj), rng.uniform(rlo, rhi, nobj)

    def tested(x, y, r):
        lo = lambda v: np.clip(np.floor(v), 0, ns)  # noqa: E731
        hi = lambda v: np.clip(np.ceil(v) + 1, 0, ns)  # noqa: E731
        return int(np.sum(np.maximum(hi(x + r) - lo(x - r), 0) * np.maximum(hi(y + r) - lo(y - r), 0)))

    xd, yd, rd = (torch.as_tensor(v).to(dev) for v in (x, y, r))
    m.in_mask.zero_()
    res["caps"] = timed(lambda: m.mask_caps_pixels(xd, yd, rd))
    res["caps_objects"], res["caps_pixels_tested"] = nobj, tested(x, y, r)
    res["caps_pixels_per_s"] = res["caps_pixels_tested"] / (1e-3 * res["caps"]["ms"])
    res["caps_pixels_per_s_kernels"] = res["caps_pixels_tested"] / (1e-3 * res["caps"]["ms_kernels"])
    device_mask = m.in_mask.cpu().numpy()

    # the numpy restatement on this host: the same nine windows from host copies of the same block, and the first circles
    ph, fh, sh = primary.cpu().numpy(), fid.cpu().numpy(), sig.cpu().numpy()
    t0 = time.perf_counter()
    arrays = (np.zeros((nlayer, ns, ns), dtype=np.float32), np.zeros((ns, ns), dtype=np.float32), np.zeros((ns, ns), dtype=np.float32))
    for w in m.windows:
        MR.paste(arrays, w[4:], ph, fh, sh, -2e-4, 2e-4)
    mask = arrays[1] == 0
    t_paste = time.perf_counter() - t0
    k = min(nobj, max(1, args.host_objects))
    t0 = time.perf_counter()
    hmask = MR.caps(np.zeros((ns, ns), dtype=bool), x[:k], y[:k], r[:k])
    t_caps = time.perf_counter() - t0
    m.in_mask.zero_()
    m.mask_caps_pixels(x[:k], y[:k], r[:k])
    same_caps = bool(np.array_equal(m.in_mask.cpu().numpy(), hmask))
    m.in_mask.fill_(True)
    paste()
    same_paste = bool(np.array_equal(m.in_image.cpu().numpy().view(np.uint32), arrays[0].view(np.uint32)) and np.array_equal(m.in_fidelity.cpu().numpy(), arrays[1])
                      and np.array_equal(m.in_noise.cpu().numpy(), arrays[2]) and np.array_equal(m.in_mask.cpu().numpy(), mask))
    res["numpy"] = {"paste_s": t_paste, "caps_objects": k, "caps_s": t_caps, "caps_pixels_tested": tested(x[:k], y[:k], r[:k]), "host_cpus": os.cpu_count(),
                    "paste_equals_device": same_paste, "caps_equal_device": same_caps, "device_caps_pixels_set": int(device_mask.sum())}
    res["numpy"]["caps_pixels_per_s"] = res["numpy"]["caps_pixels_tested"] / t_caps
    res["numpy_paste_over_device"] = t_paste / (1e-3 * res["paste"]["ms"])
    res["numpy_caps_rate_under_device"] = res["caps_pixels_per_s"] / res["numpy"]["caps_pixels_per_s"]
    line = json.dumps(res)
    print(line)
    out = os.environ.get("METAMOSAIC_BENCH_OUT", os.path.join(ROOT, "profiles", "metamosaic_bench.json"))
    with open(out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
