#!/usr/bin/env python3
"""Developer timing of sl.bootstrap_along_strike (docs/strike.md, "Intervals per station").

The workload of tools/time_strike.py - 10^6 cells in 2000 segments of synthetic_scarp(4096), h = 100, w = 5, 35 ages,
windows of --window consecutive cells every --step cells of each segment - with every window cut into blocks of --block
consecutive cells (random cells have no strike to cut along: the ranges are handed over as integers, which is what the
library takes) and --replicates replicates, against sc_fit_strike on the same cells and windows in the same run.  Both go
through the context that holds the DEM; the library's k_profile bracket is read around each call, warm, median of --reps.
The budget is the ratio of the two device times: at most 2.  The split is taken by difference: the same call at R = 1
(stage one, the block terms, two replicates and the summary of one) against the full call."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--cells", type=int, default=10 ** 6)
ap.add_argument("--segment", type=int, default=500)
ap.add_argument("--window", type=int, default=100)
ap.add_argument("--step", type=int, default=10)
ap.add_argument("--block", type=int, default=10)
ap.add_argument("--replicates", type=int, default=1000)
ap.add_argument("--half", type=int, default=100)
ap.add_argument("--swath", type=int, default=5)
ap.add_argument("--reps", type=int, default=10)
a = ap.parse_args()


def windows(seg_start, window, step):
    """Windows of ``window`` consecutive cells every ``step`` cells of each segment: (seg_win_start, win_lo, win_hi)."""
    lo, hi, start = [], [], [0]
    for s0, s1 in zip(seg_start[:-1], seg_start[1:]):
        first = np.arange(s0, max(s0 + 1, s1 - window + 1), step, dtype=np.int64)
        lo.append(first)
        hi.append(np.minimum(first + window, s1))
        start.append(start[-1] + len(first))
    return np.array(start, dtype=np.int64), np.concatenate(lo), np.concatenate(hi)


def blocks(lo, hi, block):
    """Blocks of ``block`` consecutive cells of every window: (win_blk_start, blk_hi)."""
    nb = (hi - lo + block - 1) // block
    start = np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
    k = np.arange(start[-1]) - np.repeat(start[:-1], nb)
    return start, np.minimum(np.repeat(lo, nb) + (k + 1) * block, np.repeat(hi, nb)).astype(np.int64)


def main():
    import profile_reference as pr
    import scarplet_amd as sl
    from scarplet_amd import _plan, segments
    from scarplet_amd.core import _context
    z = pr.synthetic_z(a.n)
    rng = np.random.default_rng(1)
    cells = rng.integers(0, z.size, a.cells)
    ang = 0.2 + 0.1 * rng.standard_normal(a.cells)
    lab = np.arange(a.cells) // a.segment + 1
    ages = _plan.age_grid()
    sl.Matcher(sl.DEMGrid.from_array(z, 1.0))           # the DEM on the device: the routes without an upload
    ctx = _context(0)
    sargs = segments.check_args(z.shape, 1.0, cells, lab, ang, float(a.half), float(a.swath), ages, 1.0, 20, 1)
    idx, sa, ca, seg_start, seg_label = sargs.cells, sargs.sa, sargs.ca, sargs.seg_start, sargs.seg_label
    sws, lo, hi = windows(seg_start, a.window, a.step)
    wbs, bhi = blocks(lo, hi, a.block)

    def boot(R):
        return lambda: ctx.strike_bootstrap(idx, sa, ca, seg_start, seg_label, sws, lo, hi, wbs, bhi, sargs.ages, a.half, a.swath,
                                            0, 1.0, 20, 1, 5, R, 0.95, 7)[0]
    fit = "fit_along_strike window %d step %d" % (a.window, a.step)
    full = "bootstrap_along_strike R = %d" % a.replicates
    one = "bootstrap_along_strike R = 1"
    runs = {fit: lambda: ctx.fit_strike(idx, sa, ca, seg_start, seg_label, sws, lo, hi, sargs.ages, a.half, a.swath, 0, 1.0, 1.0,
                                        20, 1)[0],
            full: boot(a.replicates), one: boot(1)}
    dev_ms = {}
    for name, run in runs.items():
        out = run()                                    # warm-up (buffers sized)
        wall, dev = [], []
        for _ in range(a.reps):
            ctx.profile(1)
            ms0 = ctx.profile_get()["k_profile"][1]
            t = time.perf_counter()
            run()
            wall.append(time.perf_counter() - t)
            dev.append(ctx.profile_get()["k_profile"][1] - ms0)
            ctx.profile(0)
        dev_ms[name] = float(np.median(dev))
        print("%-42s k_profile device time %.2f ms (median of %d, warm; min %.2f, max %.2f); wall %.2f ms (min %.2f, max %.2f); %d of %d rows done"
              % (name, dev_ms[name], a.reps, min(dev), max(dev), 1e3 * float(np.median(wall)), 1e3 * min(wall), 1e3 * max(wall), int((out["status"] != 1).sum()),
                 len(out)))
    print("%d cells of %d x %d in %d segments of %d, h %d, w %d, %d ages; %d windows of %d cells every %d, %d blocks of %d cells"
          % (a.cells, a.n, a.n, lab[-1], a.segment, a.half, a.swath, len(ages), len(lo), a.window, a.step, len(bhi), a.block))
    print("split by difference: stage one, the block terms and the summary (the call at R = 1) %.2f ms; the %d replicates of "
          "the budgeted call %.2f ms" % (dev_ms[one], a.replicates, dev_ms[full] - dev_ms[one]))
    ratio = dev_ms[full] / dev_ms[fit]
    print("bootstrap_along_strike / fit_along_strike device time: %.2f (budget: at most 2)%s"
          % (ratio, "" if ratio <= 2 else " - MISSED, see the split above"))


if __name__ == "__main__":
    main()
