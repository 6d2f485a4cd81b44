#!/usr/bin/env python3
"""Developer timing: continuous ages (refine=) of sl.fit_profiles against the plain call on the same 10^6 cells of
synthetic_scarp(4096) at h = 100, w = 5, 35 ages, and against the plain call at 64 ages, in the same run.

All calls go through a Matcher that holds the DEM on the device; the library's k_profile bracket (HIP events around every
kernel of every chunk, every call sampled) is read around each call, warm, median of --reps.  The budget of
docs/profiles.md is the ratio of the device times to the plain call at A = 64: at most 2 (1 + 3 R).

The split of a round.  refine=0 is the cut and the grid fit in k_pf_refine, and t(R) - t(0) is what the rounds cost.  A cell
whose end left the grid runs no round for that end, and a workgroup waits for the cell that runs the most of its four, so the
rounds are counted from the table (status_fine) and the cost of one is (t(2) - t(0)) / (2 x the searches a workgroup waits
for): 64 candidate fits with the erf column evaluated in each of pf_candidate's four sweeps.  The same 64 calls of
pf_candidate on a column READ from the table are a round of the centre shift's search: (t(max_shift = 8) - t(max_shift = 0))
/ 9, ten rounds against one.  The difference of the two is what evaluating the column costs.  --on-scarp takes the cells
from the scarp's line, where nearly every end has its rounds."""
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
ap.add_argument("--half", type=int, default=100)
ap.add_argument("--swath", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--on-scarp", action="store_true", help="cells within a few cells of the scarp's line: every end has its rounds")
a = ap.parse_args()


def main():
    import profile_reference as pr
    import scarplet_amd as sl
    from scarplet_amd import _lib, _plan
    from scarplet_amd.core import _context
    z = pr.synthetic_z(a.n)
    rng = np.random.default_rng(1)
    cells = pr.scarp_cells(a.n, a.cells, rng, spread=3.0) if a.on_scarp else rng.integers(0, z.size, a.cells)
    ang = 0.2 + 0.1 * rng.standard_normal(a.cells)
    ages = _plan.age_grid()
    ages64 = 10 ** np.linspace(0, 3.4, 64)
    m = sl.Matcher(sl.DEMGrid.from_array(z, 1.0))      # the DEM on the device: the routes without an upload
    ctx = _context(0)
    prof = lambda **kw: m.fit_profiles(cells, float(a.half), float(a.swath), angle=ang, min_samples=20, **kw)
    runs = {"plain, 35 ages": lambda: prof(),
            "plain, 64 ages": lambda: prof(ages=ages64),
            "refine=0": lambda: prof(refine=0),
            "refine=1": lambda: prof(refine=1),
            "refine=2": lambda: prof(refine=2),
            "max_shift=0": lambda: prof(max_shift=0.0),
            "max_shift=8": lambda: prof(max_shift=8.0)}
    dev_ms, trips = {}, {}
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
        print("%-16s k_profile device time %9.2f ms (median of %d, warm; min %.2f, max %.2f); wall %.1f ms; %d of %d rows fitted"
              % (name, dev_ms[name], a.reps, min(dev), max(dev), 1e3 * float(np.median(wall)), int((out["status"] != 1).sum()),
                 len(out)), flush=True)
        if "kt_fine" in out.dtype.names and not name.endswith("0"):
            fit = out["status"] != 1
            print("%-16s kt_fine off the grid in %d rows; status_fine 2 in %d, 4 in %d; sse_fine / sse: median %.6f"
                  % ("", int((out["kt_fine"][fit] != out["kt"][fit]).sum()), int((out["status_fine"][fit] & 2 != 0).sum()),
                     int((out["status_fine"][fit] & 4 != 0).sum()), float(np.median(out["sse_fine"][fit] / out["sse"][fit]))))
            # searches a cell runs (the minimum, and an end unless it left the grid), and what a workgroup waits for: the
            # most of its four cells (input cells 4 g .. 4 g + 3; a chunk is a multiple of four)
            n = np.where(fit, 1 + (out["status_fine"] & 2 == 0) + (out["status_fine"] & 4 == 0), 0)
            pad = np.concatenate([n, np.zeros(-len(n) % 4, dtype=n.dtype)]).reshape(-1, 4)
            trips[name] = (float(n.mean()), float(pad.max(axis=1).mean()))
            print("%-16s searches a cell: %.2f of 3; the most of a workgroup's four cells: %.2f" % (("",) + trips[name]))
    h, K = a.half, a.cells
    print("%d cells of %d x %d, h %d, w %d: %d points a profile, 64 candidates a round, four sweeps a candidate"
          % (K, a.n, a.n, h, a.swath, 2 * h + 1))
    base = dev_ms["plain, 64 ages"]
    for R in (1, 2):
        r = dev_ms["refine=%d" % R]
        print("refine=%d / plain at 64 ages, device time: %.2f (budget: at most 2 (1 + 3 R) = %d); / plain at 35 ages: %.2f"
              % (R, r / base, 2 * (1 + 3 * R), r / dev_ms["plain, 35 ages"]))
    tab_round = (dev_ms["max_shift=8"] - dev_ms["max_shift=0"]) / 9.0
    print("the cut and the grid fit (refine=0) %.2f ms; nominally (t(R) - t(0)) / (3 R) = %.2f ms a round from R = 2, %.2f from R = 1"
          % (dev_ms["refine=0"], (dev_ms["refine=2"] - dev_ms["refine=0"]) / 6.0, (dev_ms["refine=1"] - dev_ms["refine=0"]) / 3.0))
    # ... but a workgroup runs the searches of the cell that has the most of its four (R rounds each)
    erf_round = (dev_ms["refine=2"] - dev_ms["refine=0"]) / (2.0 * trips["refine=2"][1])
    evals = 4.0 * 64 * (2 * h + 1) * K
    print("split: a round of 64 candidates that a workgroup waits for (%.2f searches a workgroup, not 3) %.2f ms, of which the "
          "sweeps on a column that is read %.2f ms (a round of the shift search) and the erf %.2f ms = %.0f %%"
          % (trips["refine=2"][1], erf_round, tab_round, erf_round - tab_round, 100.0 * (erf_round - tab_round) / erf_round))
    print("%.3g erf a round: %.2f T erf/s over the device; every cell with all its searches would cost %.0f ms at R = 1 (%.1f x "
          "plain at 64 ages) and %.0f ms at R = 2 (%.1f x)"
          % (evals, evals / (erf_round - tab_round) / 1e9, dev_ms["refine=0"] + 3 * erf_round,
             (dev_ms["refine=0"] + 3 * erf_round) / base, dev_ms["refine=0"] + 6 * erf_round, (dev_ms["refine=0"] + 6 * erf_round) / base))
    assert _lib.K_NAMES[_lib.K_PROFILE] == "k_profile"


if __name__ == "__main__":
    main()
