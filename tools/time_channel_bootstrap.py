#!/usr/bin/env python3
"""Developer timing: sl.bootstrap_channel_segments (docs/channels.md, "Intervals per reach") in both depth modes against
sl.fit_channel_segments in the same mode on the same cells - the 10^6 cells of tools/time_channel_segments.py:
synthetic_channel(4096), 2000 reaches of 500 cells, h = 100, w = 5, 35 frequencies, D = 8 cells - at R = 1000 with blocks of
10 cells, in the same run.

Per mode three calls go through the context that holds the DEM on the device and are taken in turns, --reps times each, warm:
  fit_channel_segments              the yardstick: stage one, the segmented sums, (segment mode) the residual pass, the choice
  bootstrap_channel_segments, R     stage one, the block terms, R + 1 replicates a reach, the summary
  bootstrap_channel_segments, 1     the same at R = 1: the split by difference
The library's k_profile bracket (HIP events around every kernel of every chunk) is read around each call.  The budget of
docs/channels.md: the bootstrap at most twice the yardstick's mean."""
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
ap.add_argument("--block", type=int, default=10)
ap.add_argument("--half", type=int, default=100)
ap.add_argument("--swath", type=int, default=5)
ap.add_argument("--shift", type=int, default=8)
ap.add_argument("--freqs", type=int, default=35)
ap.add_argument("--replicates", type=int, default=1000)
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
    for mode in ("profile", "segment"):
        s = channel_segments.check_args((m.ny, m.nx), m.de, cells, labels, ang, float(a.half), freqs, float(a.swath), D, mode, 1.0,
                                        20, 1)
        # blocks of --block consecutive cells of each reach, handed over as CSR (random cells have no strike to cut along)
        blk_start = np.unique(np.concatenate([np.arange(s0, s1, a.block) for s0, s1 in zip(s.seg_start[:-1], s.seg_start[1:])]
                                             + [[len(s.cells)]])).astype(np.int64)
        seg_blk_start = np.searchsorted(blk_start[:-1], s.seg_start).astype(np.int64)

        def boot(R):
            return ctx.channel_bootstrap(s.cells, s.sa, s.ca, s.seg_start, s.seg_label, seg_blk_start, blk_start, s.frequencies, s.h,
                                         s.w, s.D, s.mode, s.de, s.min_samples, s.min_profiles, 5, R, 0.95, 0)[0]
        runs = {"fit_channel_segments": lambda: channel_segments._run(ctx, s, m.nx, False, False, False),
                "bootstrap_channel_segments, R = %d" % a.replicates: lambda: boot(a.replicates),
                "bootstrap_channel_segments, R = 1": lambda: boot(1)}
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
        print("depth = %r: %d cells of synthetic_channel(%d) in %d reaches, blocks of %d cells (%d blocks), h %d, w %d, %d "
              "frequencies, D %d, R %d" % (mode, a.cells, a.n, a.reaches, a.block, len(blk_start) - 1, a.half, a.swath, a.freqs,
                                           a.shift, a.replicates))
        for name in runs:
            t = out[name]
            print("  %-38s k_profile device time: mean %.2f ms of %d (%s), spread %.2f; wall %.1f ms; %d of %d rows done"
                  % (name, float(np.mean(dev[name])), a.reps, ", ".join("%.2f" % v for v in dev[name]),
                     max(dev[name]) - min(dev[name]), 1e3 * float(np.median(wall[name])), int((t["status"] & 1 == 0).sum()), len(t)))
        full, one = (float(np.mean(dev["bootstrap_channel_segments, R = %d" % r])) for r in (a.replicates, 1))
        base = float(np.mean(dev["fit_channel_segments"]))
        print("  split by difference: stage one, block terms and summary (the R = 1 call) %.2f ms; the replicates %.2f ms"
              % (one, full - one))
        r = full / base
        print("  bootstrap_channel_segments / fit_channel_segments, %s: %.3f (%s the budget of 2)"
              % (mode, r, "inside" if r <= 2.0 else "OUTSIDE"))
        b, f = out["bootstrap_channel_segments, R = %d" % a.replicates], out["fit_channel_segments"]
        done = b["status"] & 1 == 0
        print("  replicate 0 is the fit's index in %d of %d reaches; interval widths in grid steps: pooled mean %.2f, bootstrap "
              "mean %.2f" % (int((b["f_index0"][done] == f["f_index"][done]).sum()), int(done.sum()),
                             float(np.mean(f["hi_index"][done] - f["lo_index"][done] + 1)),
                             float(np.mean(b["hi_index"][done] - b["lo_index"][done] + 1))))
    assert _lib.K_NAMES[_lib.K_PROFILE] == "k_profile"


if __name__ == "__main__":
    main()
