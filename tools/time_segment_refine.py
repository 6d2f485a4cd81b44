#!/usr/bin/env python3
"""Developer timing: continuous ages (refine=) of sl.fit_segments against sl.fit_profiles(..., refine=R) on the same cells and
against the plain sl.fit_segments, in the same run: 10^6 cells of synthetic_scarp(4096) in 2000 segments at h = 100, w = 5,
35 ages, R = 1 and 2 - random cells, or with --on-scarp cells within three cells of the scarp's line.

All calls run on the DEM a Matcher holds on the device; the library's k_profile bracket (HIP events around every kernel of
every chunk, every call sampled) is read around each call, warm, median of --reps.  The budget of docs/segments.md is the
ratio of the device times: the joint call at most twice the single fits with the same R."""
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
ap.add_argument("--half", type=int, default=100)
ap.add_argument("--swath", type=int, default=5)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--on-scarp", action="store_true")
a = ap.parse_args()


def main():
    import profile_reference as pr
    import scarplet_amd as sl
    from scarplet_amd import _lib, _plan, segments
    from scarplet_amd.core import _context
    z = pr.synthetic_z(a.n)
    rng = np.random.default_rng(1)
    if a.on_scarp:
        cells = pr.scarp_cells(a.n, a.cells, rng, spread=3.0)
    else:
        cells = rng.integers(0, z.size, a.cells)
    ang = 0.2 + 0.1 * rng.standard_normal(a.cells)
    lab = np.arange(a.cells) // a.segment + 1
    ages = _plan.age_grid()
    m = sl.Matcher(sl.DEMGrid.from_array(z, 1.0))      # the DEM on the device: the routes without an upload
    ctx = _context(0)
    args = segments.check_args(z.shape, 1.0, cells, lab, ang, float(a.half), float(a.swath), ages, 1.0, 20, 1)
    seg = lambda R: segments._run(ctx, args, z.shape[1], False, False, refine=segments.check_refine(args, R))
    prof = lambda R: m.fit_profiles(cells, float(a.half), float(a.swath), angle=ang, min_samples=20, refine=R)
    runs = {"fit_segments": lambda: seg(None), "fit_segments, refine=0": lambda: seg(0)}
    for R in (1, 2):
        runs["fit_profiles, refine=%d" % R] = lambda R=R: prof(R)
        runs["fit_segments, refine=%d" % R] = lambda R=R: seg(R)
    dev_ms = {}
    for name, run in runs.items():
        out = run()                                    # warm-up (buffers sized)
        wall, dev, launches = [], [], 0
        for _ in range(a.reps):
            ctx.profile(1)
            n0, ms0 = ctx.profile_get()["k_profile"][:2]
            t = time.perf_counter()
            run()
            wall.append(time.perf_counter() - t)
            n1, ms1 = ctx.profile_get()["k_profile"][:2]
            dev.append(ms1 - ms0)
            launches = n1 - n0
            ctx.profile(0)
        dev_ms[name] = float(np.median(dev))
        fit = out["status"] != 1
        print("%-26s k_profile device time %.2f ms (median of %d, warm; min %.2f, max %.2f), %d launches; wall %.2f ms; %d of %d rows fitted"
              % (name, dev_ms[name], a.reps, min(dev), max(dev), launches, 1e3 * float(np.median(wall)), int(fit.sum()), len(out)),
              flush=True)
        if "kt_fine" in out.dtype.names:
            print("%-26s kt_fine off the grid in %d rows; an end off the grid (status_fine 2 or 4) in %d"
                  % ("", int((out["kt_fine"][fit] != out["kt"][fit]).sum()), int((out["status_fine"][fit] & 6 != 0).sum())))
    h, A, K = a.half, len(ages), a.cells
    for R in (0, 1):
        per = 8 * ((2 * h + 1) + 4 * (A + (_lib.SEGMENT_REFINE_COLUMNS if R else 0)))
        print("parked with refine %s: %d bytes a cell, %.2f GB: %d chunks of at most %d cells"
              % ("> 0" if R else "= 0", per, K * per / 1e9, -(-K * per // _lib.SEGMENT_MAX_PARK), _lib.segment_refine_cap(h, A, R)))
    print("%d cells of %d x %d (%s) in %d segments of %d, h %d, w %d, %d ages"
          % (K, a.n, a.n, "on the scarp" if a.on_scarp else "random", lab[-1], a.segment, h, a.swath, A))
    for R in (1, 2):
        s, p = dev_ms["fit_segments, refine=%d" % R], dev_ms["fit_profiles, refine=%d" % R]
        print("refine=%d: fit_segments / fit_profiles, device time: %.2f (budget: at most 2); the rounds (over refine=0): %.2f ms, "
              "%.2f ms a round" % (R, s / p, s - dev_ms["fit_segments, refine=0"], (s - dev_ms["fit_segments, refine=0"]) / (2 * R)))
    print("fit_segments, refine=0 / fit_segments, device time: %.2f" % (dev_ms["fit_segments, refine=0"] / dev_ms["fit_segments"]))
    assert _lib.K_NAMES[_lib.K_PROFILE] == "k_profile"


if __name__ == "__main__":
    main()
