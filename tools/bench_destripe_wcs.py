"""Destriping with pairs formed from WCSs (seam 21) beside the two ways that keep positions, on the mosaic of tools/bench_destripe.py: --nsca
SCAs (default 6) of side --nside (default 4088) on a ring, every SCA overlapping its two ring neighbours in both directions (2 * nsca ordered
pairs), rolled by 0, 7, -5, 15, -12, 3 degrees (cycled).  Here the geometry is made of WCSs: TAN-SIP headers at 0.11 arcsec a pixel with cubic
SIP terms of 0.4 pixels at the chip's edge, the chip centres on a hexagon whose side is a third of a chip.  The same WCSs serve the three
engines:

    stored    set_pair(wcs=, keep_positions=True): two float64 arrays a pair, formed once by imcom_wcs_pix2pix and read by every pass
    lattice   set_pair(lattice=): map_sca2sca's values at 17 x 17 Chebyshev-Lobatto nodes (an approximation, INTEGRATION.md seam 8)
    formed    set_pair(wcs=, keep_positions=False): nothing kept; wcs_pix2pix runs in the kernels

Per engine: ms of the N_eff pass (the pairs already registered on the device) and of one ``cost`` + ``residual`` pair after warm-up, the
plan's bytes, and whether formed equals stored bit for bit.  Beside them: ``effective_gain`` at --nside against the numpy restatement
(tests/destripe_setup_reference.py) on this host, and -- from the byte plan alone, no device -- the largest mosaic of 4088^2 SCAs that
``plan()`` admits into 0.9 of 288 GB with 4, 8 and 12 neighbours an SCA, stored against formed.  Writes profiles/destripe_wcs_bench.json.

    PYTHONPATH=. python tools/bench_destripe_wcs.py [--reps 3] [--warmup 1] [--nside 4088] [--nsca 6] [--plan-only] [--no-numpy]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pyimcom_amd import destripe  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--nside", type=int, default=4088)
ap.add_argument("--nsca", type=int, default=6)
ap.add_argument("--amp-cols", type=int, default=511)
ap.add_argument("--plan-only", action="store_true")
ap.add_argument("--no-numpy", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "destripe_wcs_bench.json"))
a = ap.parse_args()
n, ns = a.nside, a.nsca
ROLL = [0.0, 7.0, -5.0, 15.0, -12.0, 3.0]
S = 0.11 / 3600.0
ROOM = 0.9 * 288e9


def largest_mosaic(k, formed):
    """The most SCAs of 4088^2 with k neighbours each whose plan fits ROOM."""
    def total(m):
        return destripe.memory_plan(m, 4088, 4088, 511, n_full=0 if formed else m * k, n_lattice=0, L=0, max_np=k, n_wcs=m * k if formed else 0, gain_setup=formed)["total"]

    lo, hi = 1, 4096
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if total(mid) <= ROOM else (lo, mid - 1)
    return lo


result = {"bench": "destripe_wcs", "nside": n, "n_sca": ns, "room_bytes": ROOM, "formed_pair_bytes": destripe.formed_pair_bytes(4088),
          "largest_mosaic_4088": {str(k): {"stored": largest_mosaic(k, False), "formed": largest_mosaic(k, True)} for k in (4, 8, 12)}}
if a.plan_only:
    print(json.dumps(result))
    sys.exit(0)

import torch  # noqa: E402

from pyimcom_amd import wcs as W  # noqa: E402

dev = torch.device("cuda:0")
gen = torch.Generator(device=dev).manual_seed(8)
rng = np.random.default_rng(8)


def header(k):
    th, c = np.deg2rad(ROLL[k % 6]), np.deg2rad(360.0 * k / ns)
    half, r = n / 2.0, n / 3.0 * S  # (the hexagon's side equals its radius)
    h = {"CTYPE1": "RA---TAN-SIP", "CTYPE2": "DEC--TAN-SIP", "CRPIX1": (n + 1) / 2, "CRPIX2": (n + 1) / 2,
         "CRVAL1": 150.0 + r * np.cos(c) / np.cos(np.deg2rad(2.2)), "CRVAL2": 2.2 + r * np.sin(c),
         "CD1_1": -S * np.cos(th), "CD1_2": S * np.sin(th), "CD2_1": S * np.sin(th), "CD2_2": S * np.cos(th), "A_ORDER": 3, "B_ORDER": 3}
    for key, px in (("A_3_0", 0.4), ("A_1_2", -0.4), ("A_0_2", 0.1), ("B_0_3", 0.4), ("B_2_1", 0.4), ("B_1_1", -0.1)):
        h[key] = px * (1.0 + 0.05 * k) / half ** (int(key[2]) + int(key[4]))
    return {k_: float(v) if not isinstance(v, str) else v for k_, v in h.items()}


ws = [W.DeviceWCS.from_header(header(k), array_shape=(n, n)) for k in range(ns)]
scas = [(100.0 + 5.0 * torch.randn((n, n), dtype=torch.float32, device=dev, generator=gen), torch.rand((n, n), device=dev, generator=gen) > 0.03,
         1.0 + 0.05 * torch.randn((n, n), dtype=torch.float32, device=dev, generator=gen)) for _ in range(ns)]
pairs = sorted({(k, b) for k in range(ns) for b in ((k + 1) % ns, (k - 1) % ns) if b != k})
nodes = destripe.lattice_nodes(n, 17)[0]
gx, gy = np.meshgrid(nodes, nodes)
amp = a.amp_cols if n % a.amp_cols == 0 else None


def build(kind):
    eng = destripe.DestripeEngine(n, n, amp_cols=amp, col_boundary_const=1.0 if amp else 0.0)
    for s in scas:
        eng.add_sca(*s)
    for k, b in pairs:
        if kind == "lattice":
            x, y, _, _ = W._pix2pix(ws[k], ws[b], points=np.stack((gx.ravel(), gy.ravel()), 1), nside=n)
            eng.set_pair(k, b, lattice=torch.stack((x.reshape(17, 17), y.reshape(17, 17))))
        else:
            eng.set_pair(k, b, wcs=(ws[k], ws[b]), keep_positions=kind == "stored")
    return eng


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


params = torch.as_tensor(rng.standard_normal((ns, n + (n // amp if amp else 0))), device=dev)
kept = {}
for kind in ("stored", "lattice", "formed"):
    eng = build(kind)
    plan = eng.plan()
    ms_setup, _ = clock(lambda: eng.N_eff)

    def neff_again():
        eng._tables = None  # the pair table is made again; the pairs' arrays are on the device already
        return eng.N_eff

    ms_neff = min(clock(neff_again)[0] for _ in range(a.reps))
    for _ in range(a.warmup):
        eng.residual(eng.cost(params, "quadratic")[1], "quadratic")
    runs = []
    for _ in range(a.reps):
        t_cost, (eps, psi) = clock(lambda: eng.cost(params, "quadratic"))
        t_res, res = clock(lambda: eng.residual(psi, "quadratic"))
        runs.append((t_cost + t_res, t_cost, t_res))
    best = min(runs)
    kept[kind] = (eng.N_eff.clone(), eps, psi.clone(), res)
    result[kind] = {"ordered_pairs": eng.n_pairs, "plan_bytes": plan["total"], "pair_bytes": plan["pairs_full"] + plan["pairs_lattice"] + plan["pairs_wcs"] + plan["wcs"],
                    "ms_upload_and_first_neff": round(ms_setup, 2), "ms_neff": round(ms_neff, 2), "ms_cost_plus_residual": [round(r[0], 2) for r in runs],
                    "ms_cost": round(best[1], 2), "ms_residual": round(best[2], 2), "epsilon": eps, "overlap_fraction": round(float((kept[kind][0] > 0).double().mean()), 3)}
    del eng
    torch.cuda.empty_cache()
f, s = kept["formed"], kept["stored"]
result["formed_equals_stored"] = bool(torch.equal(f[0], s[0]) and f[1] == s[1] and torch.equal(f[2], s[2]) and np.array_equal(f[3], s[3]))
result["lattice_max_neff_difference"] = float((kept["lattice"][0] - s[0]).abs().max())
del kept

ms_gain = min(clock(lambda: destripe.effective_gain(ws[1], n, device_out=True))[0] for _ in range(a.reps + 1))
result["effective_gain"] = {"ms_device": round(ms_gain, 2)}
if not a.no_numpy:
    from tests import destripe_setup_reference as R

    t0 = time.perf_counter()
    g = R.np_effective_gain(ws[1].descriptor, None, n, np.float32)
    result["effective_gain"]["ms_numpy_restatement_same_host"] = round((time.perf_counter() - t0) * 1e3, 1)
    d = destripe.effective_gain(ws[1], n)
    result["effective_gain"]["float32_values_that_differ"] = int(np.count_nonzero(d != g))
    result["effective_gain"]["largest_relative_difference"] = float(np.max(np.abs(d.astype(np.float64) - g) / g))
print(json.dumps(result))
with open(a.out, "w") as fh:
    json.dump(result, fh, indent=1)
    fh.write("\n")
