"""One layer of the long-range PSF subtraction (pyimcom_amd.imsubtract, csrc/imsubtract.hip) at the production shape: nside 4088, oversamp 8,
Nl 4 (16 Legendre planes), canvas on the device.  ``axis_num`` is not set by the configuration: splitpsf.py writes kernel planes of the
side of the input PSF cube (``largestamp_size``, splitpsf.py:193, 249); 512 is ASSUMED here (--ax changes it).  Prints one JSON line: ms of
``LongRangeSubtractor.subtract`` per repeat after warm-up, the bytes and flops of the layer and the fraction of the float64 vector peak
(the route's roof: every multiply-add is a float64 FMA).

    PYTHONPATH=. python tools/bench_imsubtract.py [--reps 3] [--warmup 1] [--nside 4088] [--ax 512] [--nl 4]

With --cpu the reference-shaped loop (tests/imsubtract_reference.kh_full with a float32 KH: float64 FFT convolution per term at full
resolution, then the decimation) is timed on this host at the given, smaller shape instead; nothing runs on the device."""
import argparse
import json
import os
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--nside", type=int, default=4088)
ap.add_argument("--oversamp", type=int, default=8)
ap.add_argument("--ax", type=int, default=512)
ap.add_argument("--nl", type=int, default=4)
ap.add_argument("--cpu", action="store_true")
a = ap.parse_args()
nside, s, ax, Nl = a.nside, a.oversamp, a.ax, a.nl
PEAK_F64_VECTOR = 78.6e12  # MI355X: 256 CUs x 4 SIMDs x 16 lanes x 2 flop x 2.4 GHz

rng = np.random.default_rng(8)
g = np.mgrid[:ax, :ax] - (ax - 1) / 2.0
K = (0.02 * rng.standard_normal((Nl * Nl, ax, ax)) + 0.2 / (1.0 + (g[0] ** 2 + g[1] ** 2) / ax)).astype(np.float32)
flops = 2.0 * nside * nside * ax * ax * Nl * Nl

if a.cpu:
    from tests import imsubtract_reference as ref

    _, _, A = ref.geometry(ax, s, nside)
    canvas = (1.0 + 0.3 * rng.standard_normal((A, A), dtype=np.float32)).astype(np.float32)
    t0 = time.perf_counter()
    ref.kh_full(canvas, K, s, nside, Nl, dtype=np.float32)
    print(json.dumps({"bench": "imsubtract_layer_cpu_restatement", "nside": nside, "oversamp": s, "axis_num": ax, "Nl": Nl, "canvas_side": A,
                      "s_layer": round(time.perf_counter() - t0, 2), "host_threads": int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count(),
                      "note": "scipy.signal.fftconvolve per term in one piece (the reference cuts it into six bands), one FFT worker"}))
    raise SystemExit(0)

import torch

from pyimcom_amd import imsubtract

dev = torch.device("cuda:0")
I_pad, first, A = imsubtract.geometry(ax, s, nside)
canvas = 1.0 + 0.3 * torch.randn((A, A), dtype=torch.float32, device=dev, generator=torch.Generator(device=dev).manual_seed(8))
image = torch.zeros((nside, nside), dtype=torch.float32, device=dev)
t0 = time.perf_counter()
sub = imsubtract.LongRangeSubtractor(K, s, nside, -1, device=dev)
torch.cuda.synchronize()
s_prepare = time.perf_counter() - t0
for _ in range(a.warmup):
    sub.subtract(image, canvas)
torch.cuda.synchronize()
ms = []
for _ in range(a.reps):
    t0 = time.perf_counter()
    sub.subtract(image, canvas)
    torch.cuda.synchronize()
    ms.append((time.perf_counter() - t0) * 1e3)
best = min(ms)
print(json.dumps({"bench": "imsubtract_layer", "nside": nside, "oversamp": s, "axis_num": ax, "axis_num_assumed": True, "Nl": Nl, "canvas_side": A,
                  "canvas_bytes": 4 * A * A, "kernel_bytes_resident": int(sub.kf.numel()) * 8, "image_bytes": 4 * nside * nside, "flops": flops,
                  "ms_layer": [round(m, 2) for m in ms], "ms_prepare_kernel": round(s_prepare * 1e3, 2), "tflops": round(flops / best / 1e9, 2),
                  "fraction_of_f64_vector_peak": round(flops / best / 1e9 / (PEAK_F64_VECTOR / 1e12), 3),
                  "checksum": float(image.double().abs().sum().item())}))
