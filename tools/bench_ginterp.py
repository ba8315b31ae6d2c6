"""MultiInterp on a shear-image-sized call (pyimcom_amd.ginterp, csrc/ginterp.hip): 1200 x 1200 outputs, 6 float32 layers, Rsearch 6,
samp 4.71, a rotated Jacobian, input and outputs on the device.  Prints one JSON line: ms per call, output points/s and the fraction of
the fp64 matrix peak (78.6 TF/s) on the own count, per point 8 n_g^2 (corner solves) + 2 NN^2 (U) + 2 NN nlayer (gather).

    PYTHONPATH=. python tools/bench_ginterp.py [--reps 10] [--warmup 2] [--n 1200]"""
import argparse
import json

import numpy as np
import torch

from pyimcom_amd import ginterp

PEAK = 78.6e12

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--n", type=int, default=1200)
ap.add_argument("--rsearch", type=float, default=6.0)
a = ap.parse_args()

n, nl, Rs, samp, sc = a.n, 6, a.rsearch, 4.71, 0.5
sigma = samp / np.sqrt(8.0 * np.log(2.0))
th = 0.3
M = sc * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]) @ np.array([[1.0, 0.02], [0.0, 1.01]])  # sheared + rotated, half-pixel output grid
eC = (M @ M.T / sc**2 - np.identity(2)) * sigma**2 + 0.3 * np.identity(2)
C = [eC[0, 0], eC[0, 1], eC[1, 1]]
corner = M @ np.array([[0, n - 1, 0, n - 1], [0, 0, n - 1, n - 1]], dtype=np.float64)  # the output grid's corners on the input
origin = 16.0 - corner.min(axis=1)  # a margin of 16 input pixels > the search radius on every side: nothing masked
n_in = int(np.ceil((corner.max(axis=1) - corner.min(axis=1)).max())) + 33
dev = torch.device("cuda:0")
rng = np.random.default_rng(1)
img = torch.as_tensor((1.0 + 0.1 * rng.standard_normal((nl, n_in, n_in))).astype(np.float32), device=dev)
msk = torch.zeros((n_in, n_in), dtype=torch.bool, device=dev)

for _ in range(a.warmup):
    out, mask, umax, smax = ginterp.MultiInterp(img, msk, (n, n), origin, M, Rs, samp, C)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(a.reps):
    out, mask, umax, smax = ginterp.MultiInterp(img, msk, (n, n), origin, M, Rs, samp, C)
e1.record()
torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / a.reps
posx, _, corners = ginterp.geometry(Rs)
NN, ng = posx.size, corners.shape[1]
flop_pt = 8 * ng**2 + 2 * NN**2 + 2 * NN * nl
pts = n * n
print(json.dumps({"bench": "ginterp_multiinterp", "n_out": n, "nlayer": nl, "rsearch": Rs, "NN": NN, "n_g": ng, "ms": round(ms, 3),
                  "points_per_s": round(pts / ms * 1e3, 1), "kflop_per_point": round(flop_pt / 1e3, 1),
                  "tflops": round(flop_pt * pts / ms / 1e9, 2), "frac_fp64_matrix_peak": round(flop_pt * pts / ms / 1e9 / (PEAK / 1e12), 3),
                  "unmasked": float((~mask).float().mean().item()), "Umax": umax, "Smax": smax}))
