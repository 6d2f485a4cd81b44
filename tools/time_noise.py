#!/usr/bin/env python3
"""Developer timing: DEMGrid._estimate_curvature_noiselevel on a synthetic DEM.

The device time is the library's HIP-event bracket around sc_curvature_noise (profiling slot
k_noise, every call sampled); the wall time adds the host's share (the DEM upload, the NaN scan,
the 180-orientation quadratic form).  FMA rate: 2 passes x 3 planes x the taps the kernels run
(2 r + 8 rounded up to 8) per cell, against the float64 vector FMA rate of the part's spec sheet
(78.6 TFLOP/s = 39.3 T FMA/s)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from scarplet_amd import _lib, core, synthetic  # noqa: E402

SPEC_FMA_PER_S = 78.6e12 / 2

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10000)
ap.add_argument("--sigma", type=float, default=100.0)
ap.add_argument("--reps", type=int, default=2, help="calls; the first one is a warm-up")
ap.add_argument("--nan", action="store_true", help="one NaN cell in the middle (the NaN-box dilation runs too)")
a = ap.parse_args()
g = synthetic.synthetic_scarp(a.n)
if a.nan:
    g._griddata[a.n // 2, a.n // 2] = np.nan
r = int(4.0 * a.sigma + 0.5)
taps = (2 * r + 8 + 7) // 8 * 8
fma = 2 * 3 * float(a.n) * a.n * taps
ctx = core._context(0)
for rep in range(a.reps):
    if a.nan:
        g._griddata[a.n // 2, a.n // 2] = np.nan
    ctx.profile(1)
    t0 = time.time()
    angles, mean, sd = g._estimate_curvature_noiselevel(sigma=a.sigma)
    wall = time.time() - t0
    n, ms = ctx.profile_get()["k_noise"]
    print("rep %d: %dx%d sigma %g (r %d): device %.2f ms (%d bracket), wall %.3f s; %.2f T FMA/s = %.1f %% of the "
          "spec FP64 FMA rate; sd[0] %.6e sd[90] %.6e mean[0] %.3e"
          % (rep, a.n, a.n, a.sigma, r, ms, n, wall, fma / (ms * 1e-3) / 1e12, 100 * fma / (ms * 1e-3) / SPEC_FMA_PER_S,
             sd[0], sd[90], mean[0]), flush=True)
ctx.profile(0)
print("device memory held after the call: %.2f GB" % (ctx.device_bytes() / 1e9))
assert _lib.K_NAMES[_lib.K_NOISE] == "k_noise"
