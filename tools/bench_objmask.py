#!/usr/bin/env python3
"""Times the bright-object mask of pyimcom_amd.objmask on the device: ``apply_object_mask`` of one 4088 x 4088 float32 SCA with
``type="fits"`` and of one 2048 x 2048 float64 image with ``type="jwst"``, the image already on the device and the results left there;
the median of the timed repetitions after warm-up calls, by a host clock around work that ends in a device synchronise (the routes read
scalars back between their kernels, so the host's share is part of the figure), and the kernels' own time per family from the library's
event scopes.  Next to it the time of the reference's formula on the host it runs on: numpy's median, comparisons and -- when scipy is
installed -- ``binary_propagation`` / ``binary_dilation`` (``--no-host`` leaves it out; without scipy the numpy-only restatement of
tests/objmask_reference.py is timed instead and the line says so).  Prints one JSON line and writes it to profiles/objmask_bench.json.

    python tools/bench_objmask.py [--reps 5] [--warmup 2] [--no-host]"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FAMILIES = ("select_kth", "mask_flags", "mask_propagate", "mask_dilate", "mask_apply")


def scene(shape, dtype, seed, nsrc, nonfinite=0):
    """Sky noise, ``nsrc`` Gaussian sources of mixed brightness and width, a few non-finite pixels."""
    rng = np.random.default_rng(seed)
    H, W = shape
    img = (0.05 + 0.04 * rng.standard_normal(shape)).astype(dtype)
    for _ in range(nsrc):
        y, x, w = int(rng.integers(0, H)), int(rng.integers(0, W)), float(rng.uniform(1.0, 6.0))
        r = int(6 * w)
        y0, y1, x0, x1 = max(y - r, 0), min(y + r + 1, H), max(x - r, 0), min(x + r + 1, W)
        yy, xx = np.mgrid[y0:y1, x0:x1]
        img[y0:y1, x0:x1] += (float(rng.uniform(0.5, 40.0)) * np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2 * w * w))).astype(dtype)
    for k in range(nonfinite):
        img[rng.integers(0, H), rng.integers(0, W)] = (np.inf, np.nan)[k % 2]
    return img


def host_formula(image, threshold_m, threshold_c, kind):
    """(mask, which): scipy's routines as the reference calls them, or the numpy-only restatement."""
    try:
        from scipy.ndimage import binary_dilation, binary_propagation
    except ImportError:
        from tests import objmask_reference as R

        return R.apply_object_mask(image, threshold_m=threshold_m, threshold_c=threshold_c, type=kind)[1], "numpy restatement"
    ones = lambda n: np.ones((n, n), dtype=bool)  # noqa: E731
    if kind == "jwst":
        valid = np.isfinite(image)
        vals = image[valid]
        for _ in range(3):
            bkg = np.median(vals)
            sigma = 1.4826 * np.median(np.abs(vals - bkg))
            if sigma <= 0:
                break
            keep = np.abs(vals - bkg) < 3.0 * sigma
            if np.count_nonzero(keep) < 100:
                break
            vals = vals[keep]
        bkg = np.median(vals)
        sigma = 1.4826 * np.median(np.abs(vals - bkg))
        if not np.isfinite(sigma) or sigma <= 0:
            sigma = np.std(vals) if vals.size > 1 else 0.0
        with np.errstate(invalid="ignore"):
            resid = np.where(valid, image - bkg, 0)
        seed = valid & (resid >= max(threshold_c, 6.0 * sigma))
        grow = valid & (resid >= max(0.5 * threshold_c, 2.5 * sigma))
        high = binary_dilation(binary_propagation(seed, mask=grow), structure=ones(3), iterations=2)
    else:
        high = image >= threshold_m * np.median(image) + threshold_c
    return binary_dilation(high, structure=ones(5)), "numpy + scipy"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    import torch

    from pyimcom_amd import _lib, objmask

    ctx = _lib.default_context(0)
    res = {"tool": "bench_objmask", "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "source_sha16": _lib.source_sha16()}
    cases = {"fits_f32_4088": (scene((4088, 4088), np.float32, 1, 4000), 0, 0.3, "fits"),
             "jwst_f64_2048": (scene((2048, 2048), np.float64, 2, 1000, nonfinite=200), 0, 0.3, "jwst")}
    for name, (img, m, c, kind) in cases.items():
        t = torch.as_tensor(img, device="cuda:0")
        wall, kern, details = [], {f: [] for f in FAMILIES}, {}
        for i in range(args.warmup + args.reps):
            ctx.profile_enable(True)
            ctx.profile_reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, mask = objmask.apply_object_mask(t, threshold_m=m, threshold_c=c, type=kind, details=details)
            torch.cuda.synchronize()
            if i >= args.warmup:
                wall.append((time.perf_counter() - t0) * 1e3)
                for f in FAMILIES:
                    kern[f].append(ctx.profile_get(f)[0])
            ctx.profile_enable(False)
        res[name] = {"shape": list(img.shape), "dtype": str(img.dtype), "type": kind, "ms": statistics.median(wall), "ms_min": min(wall), "ms_max": max(wall),
                     "ms_kernels": {f: statistics.median(v) for f, v in kern.items()}, "masked_fraction": float(mask.sum().item()) / img.size,
                     "sweeps": details.get("sweeps")}
        if not args.no_host:
            t0 = time.perf_counter()
            host_mask, which = host_formula(img, m, c, kind)
            res[name]["s_host"], res[name]["host_formula"] = time.perf_counter() - t0, which
            res[name]["host_mask_equal"] = bool(np.array_equal(host_mask, mask.cpu().numpy()))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "objmask_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
