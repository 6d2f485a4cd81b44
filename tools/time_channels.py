#!/usr/bin/env python3
"""Developer timing: sl.fit_channels (docs/channels.md) against the centre shift of sl.fit_profiles, whose work it does, on
the same 10^6 cells of synthetic_channel(4096) at h = 100, w = 5, 35 frequencies (35 ages), D = 8 cells, in the same run.

Three calls go through one Matcher that holds the DEM on the device and are taken in turns, --reps times each, warm:
  fit_profiles, max_shift   the yardstick: the same pairs, the same four sweeps over the same LDS
  fit_channels, terms 0     option "channel_terms" 0: every profile runs the four sweeps
  fit_channels, terms 1     the default: a complete profile takes ebar, gamma and See from the call's table, two sweeps
The library's k_profile bracket (HIP events around every kernel of every chunk, every call sampled) is read around each
call.  The conditions of docs/channels.md: the slow route costs no more than the yardstick's mean plus three times the
spread (max - min) of its repeats, and the fast route beats the slow one by more than that spread."""
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
ap.add_argument("--half", type=int, default=100)
ap.add_argument("--swath", type=int, default=5)
ap.add_argument("--shift", type=int, default=8)
ap.add_argument("--freqs", type=int, default=35)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()


def main():
    import scarplet_amd as sl
    from scarplet_amd import _lib, _plan, synthetic
    from scarplet_amd.core import _context
    g = synthetic.synthetic_channel(a.n)
    rng = np.random.default_rng(1)
    cells = rng.integers(0, a.n * a.n, a.cells)
    ang = 0.2 + 0.1 * rng.standard_normal(a.cells)
    ages = _plan.age_grid()[:a.freqs]
    freqs = np.sort(1.0 / (np.sqrt(2.0) * np.pi * np.geomspace(0.5, a.half / 2, a.freqs)))
    m = sl.Matcher(g)                                  # the DEM on the device: the routes without an upload
    ctx = _context(0)
    D = float(a.shift)

    def channels(terms):
        ctx.set_option("channel_terms", terms)
        try:
            return m.fit_channels(cells, float(a.half), freqs, swath=float(a.swath), max_shift=D, angle=ang, min_samples=20)
        finally:
            ctx.set_option("channel_terms", 1)
    runs = {"fit_profiles, max_shift": lambda: m.fit_profiles(cells, float(a.half), float(a.swath), ages=ages, angle=ang,
                                                              min_samples=20, max_shift=D),
            "fit_channels, terms 0": lambda: channels(0),
            "fit_channels, terms 1": lambda: channels(1)}
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
    full = int((out["fit_channels, terms 1"]["n"] == 2 * a.half + 1).sum())
    P = a.freqs * (2 * a.shift + 1)
    print("%d cells of synthetic_channel(%d), h %d, w %d, %d frequencies / ages, D %d: %d pairs a cell, %d rounds of 64 lanes; "
          "table %.1f KB, terms %.1f KB; %d profiles complete"
          % (a.cells, a.n, a.half, a.swath, a.freqs, a.shift, P, -(-P // 64), (2 * (a.half + a.shift) + 1) * a.freqs * 8 / 1e3,
             3 * P * 8 / 1e3, full))
    for name in runs:
        t = out[name]
        print("%-24s k_profile device time: mean %.2f ms of %d (%s), spread %.2f; wall %.1f ms; %d of %d rows fitted"
              % (name, float(np.mean(dev[name])), a.reps, ", ".join("%.2f" % v for v in dev[name]),
                 max(dev[name]) - min(dev[name]), 1e3 * float(np.median(wall[name])), int((t["status"] & 1 == 0).sum()), len(t)))
    assert out["fit_channels, terms 0"].tobytes() == out["fit_channels, terms 1"].tobytes()
    print("the two routes of fit_channels returned the same bytes")
    base, spread = float(np.mean(dev["fit_profiles, max_shift"])), max(dev["fit_profiles, max_shift"]) - min(dev["fit_profiles, max_shift"])
    slow, fast = float(np.mean(dev["fit_channels, terms 0"])), float(np.mean(dev["fit_channels, terms 1"]))
    print("slow route / shift call: %.3f (%.2f ms against %.2f + 3 x %.2f = %.2f: %s)"
          % (slow / base, slow, base, spread, base + 3 * spread, "inside" if slow <= base + 3 * spread else "OUTSIDE"))
    print("fast route / slow route: %.3f (%.2f ms less, the spread %.2f: %s)"
          % (fast / slow, slow - fast, spread, "faster" if slow - fast > spread else "NOT FASTER"))
    assert _lib.K_NAMES[_lib.K_PROFILE] == "k_profile"


if __name__ == "__main__":
    main()
