"""The injected star-grid layer of one SCA (pyimcom_amd.inject, csrc/inject.hip): 4088 x 4088, a 16-plane Legendre cube of 64 x 64 at
oversamp 8, the grid points of HEALPix resolution 14 within one chip side of the chip centre (a jittered lattice of 117 px spacing cut to
that circle, about 3.8 k points, as generate_star_grid searches).  Prints one JSON line: ms of star_image end to end (host positions in,
device image out), of its two device stages on their own (PSFs of the stars that reach the chip; drawing them), and -- with --numpy --
the seconds the numpy restatement of the same work (tests/inject_reference.py) takes on this host.

    PYTHONPATH=. python tools/bench_inject.py [--reps 10] [--warmup 2] [--numpy]"""
import argparse
import json
import os
import time

import numpy as np
import torch

from pyimcom_amd import inject

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--numpy", action="store_true")
a = ap.parse_args()

nside, os_, porder, ncube, spacing = 4088, 8, 3, 64, 117.0
rng = np.random.default_rng(14)
t = np.arange(-nside, 2 * nside, spacing)
xx, yy = np.meshgrid(t, t)
x, y = (xx + rng.uniform(-20, 20, xx.shape)).ravel(), (yy + rng.uniform(-20, 20, yy.shape)).ravel()
c = (nside - 1) / 2.0
inside = (x - c) ** 2 + (y - c) ** 2 <= float(nside) ** 2
x, y = x[inside], y[inside]
g = np.mgrid[:ncube, :ncube] - (ncube - 1) / 2.0
na = (porder + 1) ** 2
cube = np.zeros((na, ncube, ncube))
cube[0] = np.exp(-(g[0] ** 2 + g[1] ** 2) / (2 * 7.0**2))
cube[0] *= 64.0 / cube[0].sum()
for k in range(1, na):
    cube[k] = 0.05 * cube[0] * rng.standard_normal((ncube, ncube)) / (1 + k)
lpoly = inject.lpoly_arr(porder, (x - 2043.5) / 2044.0, (y - 2043.5) / 2044.0)
keep = inject.on_chip(x, y, nside)
dev = torch.device("cuda:0")


def timed(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / a.reps * 1e3, out


ms_all, image = timed(lambda: inject.star_image(x, y, nside, os_, cube=cube, lpoly=lpoly, scale=1.0 / 64.0))
cube_d, lp_d = torch.as_tensor(cube, device=dev), torch.as_tensor(lpoly[keep], device=dev)
xs, ys = torch.as_tensor(x[keep], device=dev), torch.as_tensor(y[keep], device=dev)
ms_psf, psfs = timed(lambda: inject.psf_from_cube(cube_d, lp_d, float(os_), 0.0, 1.0 / 64.0))
out = torch.zeros((nside, nside), dtype=torch.float64, device=dev)
ms_draw, _ = timed(lambda: inject.draw_stars(psfs, xs, ys, nside, os_, out=out))
res = {"bench": "inject_star_image", "nside": nside, "planes": na, "oversamp": os_, "grid_points": int(x.size), "on_chip": int(keep.sum()),
       "psf_shape": list(psfs.shape[1:]), "ms_star_image": round(ms_all, 3), "ms_psf_from_cube": round(ms_psf, 3), "ms_draw_stars": round(ms_draw, 3),
       "psf_write_GBps": round(psfs.numel() * 8 / ms_psf / 1e6, 1), "flux": float(image.sum().item())}
if a.numpy:
    from tests import inject_reference as ref

    t0 = time.perf_counter()
    want = ref.star_image(cube, lpoly, x, y, nside, os_, float(os_), 1.0 / 64.0)
    res["s_numpy_restatement"] = round(time.perf_counter() - t0, 3)
    res["host_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count()
    res["max_err_vs_numpy"] = float(np.max(np.abs(image.cpu().numpy() - want)) / np.max(np.abs(want)))
print(json.dumps(res))
