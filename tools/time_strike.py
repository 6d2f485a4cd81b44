#!/usr/bin/env python3
"""Developer timing of sl.fit_along_strike (docs/strike.md).

The 10^6 cells in 2000 segments of tools/time_segments.py - synthetic_scarp(4096), h = 100, w = 5, 35 ages - with windows
of --window consecutive cells every --step cells of each segment (random cells have no strike to cut along: the ranges
are handed over as integers, which is what the library takes), against sc_fit_segments on the same cells in the same
run.  Both go through the context that holds the DEM; the library's k_profile bracket is read around each call, warm,
median of --reps.  The budget is the ratio of the two device times: at most 2.  Also timed, without a budget: the same
call at a step of one cell.  The kernel split is taken by difference: the same call with one window per segment (stage
one, Spp and next to no windows) against the full call."""
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

    def strike(window, step):
        sws, lo, hi = windows(seg_start, window, step)
        return lambda: ctx.fit_strike(idx, sa, ca, seg_start, seg_label, sws, lo, hi, sargs.ages, a.half, a.swath, 0, 1.0, 1.0,
                                      20, 1)[0]
    full = "fit_along_strike window %d step %d" % (a.window, a.step)
    dense = "fit_along_strike window %d step 1" % a.window
    one = "fit_along_strike one window a segment"
    runs = {"fit_segments": lambda: segments._run(ctx, sargs, z.shape[1], False, False),
            full: strike(a.window, a.step), dense: strike(a.window, 1), one: strike(a.segment, a.segment)}
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
    print("%d cells of %d x %d in %d segments of %d, h %d, w %d, %d ages"
          % (a.cells, a.n, a.n, lab[-1], a.segment, a.half, a.swath, len(ages)))
    print("kernel split by difference: stage one and Spp (the call with one window a segment) %.2f ms; the windows of the "
          "budgeted call %.2f ms; the windows at a step of one cell %.2f ms"
          % (dev_ms[one], dev_ms[full] - dev_ms[one], dev_ms[dense] - dev_ms[one]))
    ratio = dev_ms[full] / dev_ms["fit_segments"]
    print("fit_along_strike / fit_segments device time: %.2f (budget: at most 2)%s"
          % (ratio, "" if ratio <= 2 else " - MISSED, see the split above"))
    print("at a step of one cell: %.2f" % (dev_ms[dense] / dev_ms["fit_segments"]))


if __name__ == "__main__":
    main()
