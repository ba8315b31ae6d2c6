"""One evaluation of the destriping cost and its gradient (pyimcom_amd.destripe, csrc/destripe.hip) on a synthetic mosaic: --nsca SCAs
(default 6) of side --nside (default 4088), every SCA overlapping its two ring neighbours in both directions (2 * nsca ordered pairs),
each pair a roll about the SCA centre by the difference of the roll angles 0, 7, -5, 15, -12, 3 degrees (cycled), a shift of a third of
a side and cubic terms of 0.4 pixels.  --positions full (default; float64 position arrays resident) or lattice (17 x 17 nodes per pair).
Prints one JSON line: ms of one ``cost`` + ``residual`` pair after warm-up and the fraction of the HBM peak on the tool's own byte count
-- per evaluation: cost reads image 4 + mask 1 + g_eff 4 + N_eff 8 and writes psi 4 bytes per target pixel, and per pair and target pixel
16 bytes of positions (full arrays) and, where the cell is inside, four corners of image 4 + mask 1 + g_eff 4 (counted once each: 9
bytes, neighbouring cells share lines); the gradient reads psi 4 + g_eff 4 + N_eff 8 once for term_1 and again per pair with 16 bytes of
positions and 4 bytes of g_b.  The overlap fraction is measured on the host.

    PYTHONPATH=. python tools/bench_destripe.py [--reps 3] [--warmup 1] [--nside 4088] [--nsca 6] [--positions full|lattice]"""
import argparse
import json
import time

import numpy as np
import torch

from pyimcom_amd import destripe

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--nside", type=int, default=4088)
ap.add_argument("--nsca", type=int, default=6)
ap.add_argument("--amp-cols", type=int, default=511)
ap.add_argument("--positions", default="full")
a = ap.parse_args()
n, ns = a.nside, a.nsca
HBM_PEAK = 8.0e12  # MI355X HBM3E, bytes / s
ROLL = [0.0, 7.0, -5.0, 15.0, -12.0, 3.0]
dev = torch.device("cuda:0")
gen = torch.Generator(device=dev).manual_seed(8)
rng = np.random.default_rng(8)
eng = destripe.DestripeEngine(n, n, amp_cols=a.amp_cols if n % a.amp_cols == 0 else None, col_boundary_const=1.0 if n % a.amp_cols == 0 else 0.0)
for k in range(ns):
    eng.add_sca(100.0 + 5.0 * torch.randn((n, n), dtype=torch.float32, device=dev, generator=gen),
                torch.rand((n, n), device=dev, generator=gen) > 0.03, 1.0 + 0.05 * torch.randn((n, n), dtype=torch.float32, device=dev, generator=gen))
nodes = destripe.lattice_nodes(n, 17)[0] if a.positions == "lattice" else np.arange(n, dtype=np.float64)


def pair_map(k, b, grid):
    th = np.deg2rad(ROLL[b % 6] - ROLL[k % 6])
    u, v = np.meshgrid(grid / n - 0.5, grid / n - 0.5)
    sx, sy = (n / 3.0, 0.1 * n) if b == (k + 1) % ns else (-n / 3.0, -0.1 * n)
    return ((n - 1) / 2.0 + sx + 0.237 + n * (np.cos(th) * u - np.sin(th) * v) + 0.4 * (u ** 3 - u * v ** 2 + v ** 2),
            (n - 1) / 2.0 + sy + 0.411 + n * (np.sin(th) * u + np.cos(th) * v) + 0.4 * (v ** 3 + u ** 2 * v - u * v))


inside, done = 0.0, set()
for k in range(ns):
    for b in ((k + 1) % ns, (k - 1) % ns):
        if b == k or (k, b) in done:
            continue
        done.add((k, b))
        x, y = pair_map(k, b, nodes)
        xs, ys = pair_map(k, b, np.arange(0, n, 8, dtype=np.float64))  # the overlap fraction, on every eighth pixel
        inside += float(np.mean((xs >= 0) & (ys >= 0) & (xs < n - 1) & (ys < n - 1)))
        if a.positions == "lattice":
            eng.set_pair(k, b, lattice=np.stack([x, y]))
        else:
            eng.set_pair(k, b, x=torch.as_tensor(x, device=dev), y=torch.as_tensor(y, device=dev))
npairs = eng.n_pairs
params = torch.as_tensor(rng.standard_normal((ns, eng.nbins)), device=dev)
plan = eng.plan()
t0 = time.perf_counter()
eng.N_eff
torch.cuda.synchronize()
ms_setup = (time.perf_counter() - t0) * 1e3
for _ in range(a.warmup):
    eng.residual(eng.cost(params, "quadratic")[1], "quadratic")
ms = []
for _ in range(a.reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eps, psi = eng.cost(params, "quadratic")
    t1 = time.perf_counter()
    res = eng.residual(psi, "quadratic")
    t2 = time.perf_counter()
    ms.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
best = min(ms)
px = float(n) * n
pos = 16.0 if a.positions == "full" else 0.0
frac = inside / npairs
nbytes = px * (ns * 21.0 + npairs * (pos + 9.0 * frac)) + px * (ns * 16.0 + npairs * (16.0 + pos + 4.0 * frac))
print(json.dumps({"bench": "destripe_cost_and_residual", "nside": n, "n_sca": ns, "ordered_pairs": npairs, "roll_deg": ROLL[:min(ns, 6)], "positions": a.positions,
                  "amp_cols": eng.amp_cols, "overlap_fraction": round(frac, 3), "plan_bytes": plan["total"],
                  "ms_upload_and_neff": round(ms_setup, 2), "ms_cost_plus_residual": [round(m[0], 2) for m in ms], "ms_cost": round(best[1], 2),
                  "ms_residual": round(best[2], 2), "bytes_counted": nbytes,
                  "fraction_of_hbm_peak": round(nbytes / (best[0] * 1e-3) / HBM_PEAK, 4), "hbm_peak_bytes_per_s": HBM_PEAK,
                  "epsilon": eps, "checksum": float(np.abs(res).sum())}))
