"""One exposure of the PSF split (pyimcom_amd.splitpsf.split_cubes, csrc/splitpsf.hip): 18 SCAs of 16 Legendre planes, oversamp 8, sheared
covariances, cubes on the device.  The side of the planes is not set by the configuration (it is the side of the input PSF file's
cubes); 512 is ASSUMED here (--side changes it).  Prints one JSON line: ms per exposure after warm-up, the tool's own count of the bytes
the passes move and the fraction of the HBM roof that count makes.

    PYTHONPATH=. python tools/bench_splitpsf.py [--reps 3] [--warmup 1] [--side 512] [--nsca 18] [--lorder 3]

Byte count (per SCA and grid point, N = 2 side; a complex plane is 16 N^2 bytes): four 2-D transforms of two passes, each reading and
writing a complex plane (16 x 16 N^2), the filter (2 x 16 N^2), the spectrum product (2 x 16 N^2), the two paddings (2 x 16 N^2 written)
and the crops (2 x 16 N^2 / 4 read): 340 N^2 + the side^2 passes (locLRP: npoly + 1 planes, K_real, zeta, K_Legendre: about (npoly + 8) x 8
side^2).  The tophat filter and the split (once per SCA) are counted the same way."""
import argparse
import json
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--side", type=int, default=512)
ap.add_argument("--nsca", type=int, default=18)
ap.add_argument("--lorder", type=int, default=3)
ap.add_argument("--oversamp", type=int, default=8)
a = ap.parse_args()
HBM_ROOF = 8.0e12  # MI355X: bytes per second

import torch

from pyimcom_amd import splitpsf

dev = torch.device("cuda:0")
n, nsca, npoly, s = a.side, a.nsca, (a.lorder + 1) ** 2, a.oversamp
gen = torch.Generator(device=dev).manual_seed(8)
g = torch.arange(n, dtype=torch.float64, device=dev) - (n - 1) / 2.0
r2 = g[:, None] ** 2 + g[None, :] ** 2
base = torch.exp(-r2 / 50.0) + 0.05 / (1 + r2 / 40.0) ** 1.5
cubes = base * (1 + 0.2 * torch.randn((nsca, npoly, n, n), dtype=torch.float64, device=dev, generator=gen))
cubes = cubes / base.sum()
cov = np.tile(np.array([[70.0, 3.0], [3.0, 60.0]]), (nsca, npoly, 1, 1)) * (1 + 0.01 * np.arange(nsca * npoly).reshape(nsca, npoly, 1, 1))
pars = dict(oversamp=s, smallstamp_size=min(n, 160))
top, dec = splitpsf.routes(n, s)
for _ in range(a.warmup):
    out = splitpsf.split_cubes(cubes, None, pars, covs=cov)
torch.cuda.synchronize()
ms = []
for _ in range(a.reps):
    t0 = time.perf_counter()
    out = splitpsf.split_cubes(cubes, None, pars, covs=cov)
    torch.cuda.synchronize()
    ms.append((time.perf_counter() - t0) * 1e3)
N, Nt = 2 * n, n + 2 * (-(-s // 4) * 4)
per_point = 340 * N * N + (npoly + 8) * 8 * n * n
per_sca = npoly * per_point + (npoly + 1) // 2 * (2 * 2 * 32 + 2 * 16 + 16) * Nt * Nt + 3 * npoly * 8 * n * n
total = nsca * per_sca
best = min(ms)
print(json.dumps({"bench": "splitpsf_exposure", "nsca": nsca, "npoly": npoly, "side": n, "side_assumed": a.side == 512, "oversamp": s,
                  "route_tophat": top, "route_deconvolution": dec, "ms_exposure": [round(m, 2) for m in ms], "bytes": int(total),
                  "tb_per_s": round(total / best / 1e9, 3), "fraction_of_hbm_roof": round(total / best * 1e3 / HBM_ROOF, 3),
                  "maxzeta": float(out["MAXZETA"].max().item()), "checksum": float(out["K_Legendre"].double().abs().sum().item())}))
