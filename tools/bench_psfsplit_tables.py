"""Time PSFSPLIT's wide overlap tables (imcom_psf_overlap_spectra_wide) against the narrow entry (imcom_psf_overlap_spectra_win) on the same
resident spectra, at production size (npixpsf 48, oversamp 8: PSF side 383, nfft 768, table side 767 against 383): the table sets of one
PSF group of six exposures plus a target -- 21 self, 6 input-output, 1 output self table -- whole, and windowed to what a cfg-2 batch
reads of them (separations of a stamp's input pixels: n2 + 2 INPAD = 82.6 output pixels = 157 samples either way; input-output: 124).
One warm-up, then three repeats of every variant, alternating, timed with device events.  Prints one JSON line:

    python tools/bench_psfsplit_tables.py > profiles/psfsplit_tables_bench.json

bytes: what a variant has to move at least -- every spectrum read once, every table element inside its window written once."""
import json
import sys

import numpy as np
import torch

from pyimcom_amd import synth
from pyimcom_amd.stamps import overlap_tables, psf_spectra
from pyimcom_amd._lib import default_context

HBM_PEAK = 8.0e12  # bytes / s (specification)
E, REPS = 6, 3
cfg = synth.CONFIGS["cfg2"]
ns, nfft = cfg.nsamp, cfg.nfft
ntab = 2 * ns + 1
dev = torch.device("cuda:0")
ctx = default_context()
psfs, target = synth.make_psfs(cfg, E)
allp = torch.cat([torch.as_tensor(psfs, device=dev), torch.as_tensor(target, device=dev)])
spec = psf_spectra(ctx, allp, nfft)
assert spec is not None
pairs = [(i, j) for i in range(E) for j in range(i, E)] + [(i, E) for i in range(E)] + [(E, E)]
reach_ii = int(np.ceil((cfg.n2 + 2 * cfg.inpad_as / cfg.dtheta_as) / cfg.dscale)) + 8  # samples, + the ten-tap stencil's margin
reach_io = int(np.ceil((cfg.n2 + cfg.inpad_as / cfg.dtheta_as) / cfg.dscale)) + 8


def windows(side):
    nc = side // 2
    w = []
    for q in range(len(pairs)):
        r = reach_ii if q < E * (E + 1) // 2 else (reach_io if q < len(pairs) - 1 else 8)
        lo, hi = max(0, nc - r), min(side, nc + r + 1)
        w.append((lo, hi, lo, hi))
    return np.array(w, dtype=np.int32)


variants = {}
for name, side in (("narrow", ns), ("wide", ntab)):
    for mode in ("whole", "windowed"):
        win = windows(side) if mode == "windowed" else None
        out = torch.zeros((len(pairs), side + 12, side + 12), dtype=torch.float64, device=dev)
        area = float(len(pairs) * side * side) if win is None else float(((win[:, 1] - win[:, 0]) * (win[:, 3] - win[:, 2])).sum())
        variants[f"{name}_{mode}"] = dict(side=side, win=win, out=out, bytes=spec.numel() * 8 + area * 8, ms=[])


def run(v):
    overlap_tables(ctx, None, spec, None, spec, ns, nfft, pairs, None, v["out"], win=v["win"], ntab=v["side"])


for v in variants.values():  # warm-up: workspace growth, code objects
    run(v)
torch.cuda.synchronize()
for _ in range(REPS):
    for v in variants.values():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run(v)
        b.record()
        b.synchronize()
        v["ms"].append(a.elapsed_time(b))
# the whole and the windowed tables agree on the windows (what is timed is what the tests pin)
for name in ("narrow", "wide"):
    w, full, part = variants[f"{name}_windowed"]["win"], variants[f"{name}_whole"]["out"], variants[f"{name}_windowed"]["out"]
    for q in (0, len(pairs) - 2):
        r0, r1, c0, c1 = (int(x) for x in w[q])
        assert torch.equal(full[q, 6 + r0 : 6 + r1, 6 + c0 : 6 + c1], part[q, 6 + r0 : 6 + r1, 6 + c0 : 6 + c1])
res = {"tool": "bench_psfsplit_tables", "device": torch.cuda.get_device_name(0), "npixpsf": cfg.npixpsf, "oversamp": cfg.oversamp, "nsamp": ns, "nfft": nfft,
       "ntab": ntab, "exposures": E, "tables": len(pairs), "repeats": REPS, "reach_samples": [reach_ii, reach_io]}
for k, v in variants.items():
    ms = float(np.median(v["ms"]))
    res[k] = {"ms": round(ms, 4), "ms_all": [round(x, 4) for x in v["ms"]], "us_per_table": round(ms * 1e3 / len(pairs), 2), "bytes": int(v["bytes"]),
              "hbm_roof_fraction": round(v["bytes"] / HBM_PEAK / (ms * 1e-3), 4)}
res["wide_over_narrow_whole"] = round(res["wide_whole"]["ms"] / res["narrow_whole"]["ms"], 3)
res["wide_over_narrow_windowed"] = round(res["wide_windowed"]["ms"] / res["narrow_windowed"]["ms"], 3)
res["wide_windowed_over_whole"] = round(res["wide_windowed"]["ms"] / res["wide_whole"]["ms"], 3)
json.dump(res, sys.stdout)
print()
