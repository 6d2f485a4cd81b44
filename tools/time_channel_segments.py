#!/usr/bin/env python3
"""Developer timing: sl.fit_channel_segments (docs/channels.md, "One width per reach") in both depth modes against
sl.fit_channels, whose per-cell search it runs once, on the same 10^6 cells of synthetic_channel(4096) - 2000 reaches of 500
cells - at h = 100, w = 5, 35 frequencies, D = 8 cells, in the same run.

Three calls go through one Matcher that holds the DEM on the device and are taken in turns, --reps times each, warm:
  fit_channels                      the yardstick: the same pairs on the same routes, one row per cell
  fit_channel_segments, profile     the same sweeps, the planes parked, two segmented sums of two planes and the choice
  fit_channel_segments, segment     ... and one residual sweep per frequency over the parked profiles, then a third sum
The library's k_profile bracket (HIP events around every kernel of every chunk, every call sampled) is read around each
call.  The budget of docs/channels.md: each mode at most twice the yardstick's mean."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--cells", type=int, default=10 ** 6)
ap.add_argument("--reaches", type=int, default=2000)
ap.add_argument("--half", type=int, default=100)
ap.add_argument("--swath", type=int, default=5)
ap.add_argument("--shift", type=int, default=8)
ap.add_argument("--freqs", type=int, default=35)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()


def main():
    import scarplet_amd as sl
    from scarplet_amd import _lib, channel_segments, synthetic
    from scarplet_amd.core import _context
    g = synthetic.synthetic_channel(a.n)
    rng = np.random.default_rng(1)
    cells = rng.integers(0, a.n * a.n, a.cells)
    ang = 0.2 + 0.1 * rng.standard_normal(a.cells)
    labels = np.arange(a.cells) * a.reaches // a.cells + 1           # reaches of neighbouring input cells
    freqs = np.sort(1.0 / (np.sqrt(2.0) * np.pi * np.geomspace(0.5, a.half / 2, a.freqs)))
    m = sl.Matcher(g)                                  # the DEM on the device: the routes without an upload
    ctx = _context(0)
    D = float(a.shift)

    def joint(mode):
        # (Matcher.fit_channel_segments takes the Traces of a search; the cells here are drawn, so: its two lines)
        args = channel_segments.check_args((m.ny, m.nx), m.de, cells, labels, ang, float(a.half), freqs, float(a.swath), D, mode,
                                           1.0, 20, 1)
        return channel_segments._run(m.ctx, args, m.nx, False, False, False)
    runs = {"fit_channels": lambda: m.fit_channels(cells, float(a.half), freqs, swath=float(a.swath), max_shift=D, angle=ang,
                                                   min_samples=20),
            "fit_channel_segments, profile": lambda: joint("profile"),
            "fit_channel_segments, segment": lambda: joint("segment")}
    out = {name: run() for name, run in runs.items()}  # warm-up (buffers sized)
    dev = {name: [] for name in runs}
    wall = {name: [] for name in runs}
    for _ in range(a.reps):                            # in turns: what else runs on the host meets all three alike
        for name, run in runs.items():
            ctx.profile(1)
            ms0 = ctx.profile_get()["k_profile"][1]
            t = time.perf_counter()
            run()
            wall[name].append(time.perf_counter() - t)
            dev[name].append(ctx.profile_get()["k_profile"][1] - ms0)
            ctx.profile(0)
    full = int((out["fit_channels"]["n"] == 2 * a.half + 1).sum())
    P = a.freqs * (2 * a.shift + 1)
    print("%d cells of synthetic_channel(%d) in %d reaches, h %d, w %d, %d frequencies, D %d: %d pairs a cell; park %d bytes a "
          "cell, %d cells a chunk at most; %d profiles complete"
          % (a.cells, a.n, a.reaches, a.half, a.swath, a.freqs, a.shift, P, _lib.channel_segment_park(a.half, a.freqs),
             _lib.channel_segment_cap(a.half, a.freqs), full))
    for name in runs:
        t = out[name]
        print("%-32s k_profile device time: mean %.2f ms of %d (%s), spread %.2f; wall %.1f ms; %d of %d rows fitted"
              % (name, float(np.mean(dev[name])), a.reps, ", ".join("%.2f" % v for v in dev[name]),
                 max(dev[name]) - min(dev[name]), 1e3 * float(np.median(wall[name])), int((t["status"] & 1 == 0).sum()), len(t)))
    base = float(np.mean(dev["fit_channels"]))
    for name in list(runs)[1:]:
        r = float(np.mean(dev[name])) / base
        print("%s / fit_channels: %.3f (%s the budget of 2)" % (name, r, "inside" if r <= 2.0 else "OUTSIDE"))
    t = out["fit_channel_segments, profile"]
    print("best frequency index over the fitted reaches, profile mode: %s" % np.bincount(t["f_index"][t["status"] & 1 == 0]))
    assert _lib.K_NAMES[_lib.K_PROFILE] == "k_profile"


if __name__ == "__main__":
    main()
