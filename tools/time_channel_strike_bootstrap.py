#!/usr/bin/env python3
"""Developer timing: sl.bootstrap_channels_along_strike (docs/channels.md, "Intervals per station") in both depth modes
against sl.fit_channels_along_strike in the same mode on the same cells - the 10^6 cells of tools/time_channel_strike.py:
synthetic_channel(4096), 2000 reaches of 500 cells, h = 100, w = 5, 35 frequencies, D = 8 cells - with windows of 100 cells
every 10 cells in blocks of ten cells, R = 1000.

Per mode three calls go through the context that holds the DEM on the device and are taken in turns, --reps times each, warm:
  fit_channels_along_strike                the yardstick: stage one, (segment mode) k_st_spp, k_cw_fit on 41 windows a reach
  bootstrap_channels_along_strike, R       stage one, k_cwb_window on the same windows
  bootstrap_channels_along_strike, R = 1   the same with one replicate: the split by difference
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
ap.add_argument("--step", type=int, default=10, help="cells between two windows")
ap.add_argument("--block", type=int, default=10, help="cells of a block")
ap.add_argument("--replicates", type=int, default=1000)
ap.add_argument("--half", type=int, default=100)
ap.add_argument("--swath", type=int, default=5)
ap.add_argument("--shift", type=int, default=8)
ap.add_argument("--freqs", type=int, default=35)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()


def windows(seg_start, width, step, block):
    """Windows of ``width`` consecutive cells every ``step`` cells of each reach and their blocks of ``block`` consecutive
    cells, as CSR (random cells have no strike to cut along)."""
    sws, lo, hi = [0], [], []
    for s0, s1 in zip(seg_start[:-1], seg_start[1:]):
        first = np.arange(s0, max(s0 + 1, s1 - width + 1), step)
        lo.append(first)
        hi.append(np.minimum(first + width, s1))
        sws.append(sws[-1] + len(first))
    lo, hi = np.concatenate(lo).astype(np.int64), np.concatenate(hi).astype(np.int64)
    nb = -(-(hi - lo) // block)
    wbs = np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
    k = np.arange(int(wbs[-1])) - np.repeat(wbs[:-1], nb)             # the block's number within its window
    bhi = np.minimum(np.repeat(lo, nb) + (k + 1) * block, np.repeat(hi, nb)).astype(np.int64)
    return np.array(sws, dtype=np.int64), lo, hi, wbs, np.ascontiguousarray(bhi)


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
        sws, lo, hi, wbs, bhi = windows(s.seg_start, a.window, a.step, a.block)

        def boot(R):
            return ctx.channel_strike_bootstrap(s.cells, s.sa, s.ca, s.seg_start, s.seg_label, sws, lo, hi, wbs, bhi, s.frequencies,
                                                s.h, s.w, s.D, s.mode, s.de, s.min_samples, s.min_profiles, 5, R, 0.95, 0)[0]
        runs = {"fit_channels_along_strike": lambda: ctx.channel_strike(s.cells, s.sa, s.ca, s.seg_start, s.seg_label, sws, lo, hi,
                                                                        s.frequencies, s.h, s.w, s.D, s.mode, s.de, s.delta,
                                                                        s.min_samples, s.min_profiles)[0],
                "bootstrap_channels_along_strike, R = %d" % a.replicates: lambda: boot(a.replicates),
                "bootstrap_channels_along_strike, R = 1": lambda: boot(1)}
        out = {name: run() for name, run in runs.items()}              # warm-up (buffers sized)
        dev = {name: [] for name in runs}
        wall = {name: [] for name in runs}
        for _ in range(a.reps):                        # in turns: what else runs on the host meets all three alike
            for name, run in runs.items():
                ctx.profile(1)
                ms0 = ctx.profile_get()["k_profile"][1]
                t = time.perf_counter()
                run()
                wall[name].append(time.perf_counter() - t)
                dev[name].append(ctx.profile_get()["k_profile"][1] - ms0)
                ctx.profile(0)
        print("depth = %r: %d cells of synthetic_channel(%d) in %d reaches, windows of %d cells every %d in blocks of %d, h %d, w %d, "
              "%d frequencies, D %d" % (mode, a.cells, a.n, a.reaches, a.window, a.step, a.block, a.half, a.swath, a.freqs, a.shift))
        for name in runs:
            t = out[name]
            print("  %-42s k_profile device time: mean %.2f ms of %d (%s), spread %.2f; wall %.1f ms; %d of %d rows done"
                  % (name, float(np.mean(dev[name])), a.reps, ", ".join("%.2f" % v for v in dev[name]),
                     max(dev[name]) - min(dev[name]), 1e3 * float(np.median(wall[name])), int((t["status"] & 1 == 0).sum()), len(t)))
        names = list(runs)
        base, full, one = (float(np.mean(dev[n])) for n in names)
        r = full / base
        print("  %d windows of %d blocks; split by difference: stage one and R = 1 %.2f ms, the other %d replicates %.2f ms, %.1f %% of "
              "the call; bootstrap_channels_along_strike / fit_channels_along_strike, %s: %.3f (%s the budget of 2)"
              % (len(lo), int(np.diff(wbs).max()), one, a.replicates - 1, full - one, 100.0 * (full - one) / full, mode, r,
                 "inside" if r <= 2.0 else "OUTSIDE"))
        # replicate 0 takes every block once: the window's fit
        f, b = out[names[0]], out[names[1]]
        done = (f["status"] & 1 == 0) & (b["status"] & 1 == 0)
        print("  replicate 0 is the window's fit in %d of %d windows; windows with a failed replicate: %d"
              % (int((b["f_index0"][done] == f["kt_index"][done]).sum()), int(done.sum()), int((b["n_failed"] > 0).sum())))
    lds = _lib.channel_strike_boot_lds(-(-a.window // a.block), a.freqs, a.replicates, True) + _lib.CHANNEL_STRIKE_BOOT_LDS_STATIC
    print("k_cwb_window: %d bytes of LDS a workgroup in profile mode at this workload, %d workgroups of four waves a CU by LDS"
          % (lds, _lib.LDS_BYTES // lds))
    assert _lib.K_NAMES[_lib.K_PROFILE] == "k_profile"


if __name__ == "__main__":
    main()
