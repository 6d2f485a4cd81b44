#!/usr/bin/env python3
"""Developer timing: sl.fit_channels_along_strike (docs/channels.md, "Width along a reach") in both depth modes against
sl.fit_channel_segments in the same mode on the same cells - the 10^6 cells of tools/time_channel_segments.py:
synthetic_channel(4096), 2000 reaches of 500 cells, h = 100, w = 5, 35 frequencies, D = 8 cells - with windows of 100 cells
every 10 cells, then every cell, in the same run.

Per mode four calls go through the context that holds the DEM on the device and are taken in turns, --reps times each, warm:
  fit_channel_segments                   the yardstick: stage one, the segmented sums, (segment mode) the residual pass, the choice
  fit_channels_along_strike, step 10     stage one, (segment mode) k_st_spp, k_cw_fit on 41 windows a reach
  fit_channels_along_strike, step 1      the same on 401 windows a reach
  fit_channels_along_strike, one window  the same with one window over every reach: the split by difference
The library's k_profile bracket (HIP events around every kernel of every chunk) is read around each call.  The budget of
docs/channels.md for every consumer of stage one: at most twice the yardstick's mean."""
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
ap.add_argument("--window", type=int, default=100, help="cells of a window")
ap.add_argument("--half", type=int, default=100)
ap.add_argument("--swath", type=int, default=5)
ap.add_argument("--shift", type=int, default=8)
ap.add_argument("--freqs", type=int, default=35)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()


def windows(seg_start, width, step):
    """Windows of ``width`` consecutive cells every ``step`` cells of each reach, as CSR (random cells have no strike to cut
    along); width 0: one window over the reach."""
    sws, lo, hi = [0], [], []
    for s0, s1 in zip(seg_start[:-1], seg_start[1:]):
        first = np.arange(s0, max(s0 + 1, s1 - width + 1), step) if width else np.array([s0])
        lo.append(first)
        hi.append(np.minimum(first + width, s1) if width else np.array([s1]))
        sws.append(sws[-1] + len(first))
    return np.array(sws, dtype=np.int64), np.concatenate(lo).astype(np.int64), np.concatenate(hi).astype(np.int64)


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
    for mode in ("profile", "segment"):
        s = channel_segments.check_args((m.ny, m.nx), m.de, cells, labels, ang, float(a.half), freqs, float(a.swath), D, mode, 1.0,
                                        20, 1)
        cuts = {"step 10": windows(s.seg_start, a.window, 10), "step 1": windows(s.seg_start, a.window, 1),
                "one window": windows(s.seg_start, 0, 1)}

        def along(cut):
            sws, lo, hi = cuts[cut]
            return ctx.channel_strike(s.cells, s.sa, s.ca, s.seg_start, s.seg_label, sws, lo, hi, s.frequencies, s.h, s.w, s.D,
                                      s.mode, s.de, s.delta, s.min_samples, s.min_profiles)[0]
        runs = {"fit_channel_segments": lambda: channel_segments._run(ctx, s, m.nx, False, False, False)}
        for cut in cuts:
            runs["fit_channels_along_strike, " + cut] = lambda cut=cut: along(cut)
        out = {name: run() for name, run in runs.items()}              # warm-up (buffers sized)
        dev = {name: [] for name in runs}
        wall = {name: [] for name in runs}
        for _ in range(a.reps):                        # in turns: what else runs on the host meets all four alike
            for name, run in runs.items():
                ctx.profile(1)
                ms0 = ctx.profile_get()["k_profile"][1]
                t = time.perf_counter()
                run()
                wall[name].append(time.perf_counter() - t)
                dev[name].append(ctx.profile_get()["k_profile"][1] - ms0)
                ctx.profile(0)
        print("depth = %r: %d cells of synthetic_channel(%d) in %d reaches, windows of %d cells, h %d, w %d, %d frequencies, D %d"
              % (mode, a.cells, a.n, a.reaches, a.window, a.half, a.swath, a.freqs, a.shift))
        for name in runs:
            t = out[name]
            print("  %-40s k_profile device time: mean %.2f ms of %d (%s), spread %.2f; wall %.1f ms; %d of %d rows fitted"
                  % (name, float(np.mean(dev[name])), a.reps, ", ".join("%.2f" % v for v in dev[name]),
                     max(dev[name]) - min(dev[name]), 1e3 * float(np.median(wall[name])), int((t["status"] & 1 == 0).sum()), len(t)))
        base = float(np.mean(dev["fit_channel_segments"]))
        one = float(np.mean(dev["fit_channels_along_strike, one window"]))
        for cut in ("step 10", "step 1"):
            full = float(np.mean(dev["fit_channels_along_strike, " + cut]))
            r = full / base
            print("  %s: %d windows; split by difference: stage one%s and one window a reach %.2f ms, the windows %.2f ms, %.1f %% "
                  "of the call; fit_channels_along_strike / fit_channel_segments, %s: %.3f (%s the budget of 2)"
                  % (cut, len(cuts[cut][1]), " and k_st_spp" if mode == "segment" else "", one, full - one,
                     100.0 * (full - one) / full, mode, r, "inside" if r <= 2.0 else "OUTSIDE"))
        # one window over a reach handed over in this order is the pooled fit's index
        f, w = out["fit_channel_segments"], out["fit_channels_along_strike, one window"]
        done = f["status"] & 1 == 0
        print("  one window a reach is the pooled fit's index in %d of %d reaches"
              % (int((w["kt_index"][done] == f["f_index"][done]).sum()), int(done.sum())))
    assert _lib.K_NAMES[_lib.K_PROFILE] == "k_profile"


if __name__ == "__main__":
    main()
