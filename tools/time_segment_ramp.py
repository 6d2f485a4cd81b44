#!/usr/bin/env python3
"""Developer timing: the shared initial-slope width (max_width) of sl.fit_segments, with the width free and with the slope
given, against sl.fit_profiles(..., max_width=...) and the plain sl.fit_segments on the same 10^6 cells of
synthetic_scarp(4096) in 2000 segments at h = 100, w = 5, 35 ages, M = 8 cells, in the same run.

All calls run on the DEM a Matcher holds on the device; the library's k_profile bracket (HIP events around every kernel of
every chunk, every call sampled) is read around each call, warm, median of --reps.  The budget of docs/segments.md is the
ratio of the device times: the joint call at most twice the single fits with the same width range."""
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
ap.add_argument("--width", type=int, default=8)
ap.add_argument("--slope", type=float, default=0.6)
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()


def main():
    import profile_reference as pr
    import scarplet_amd as sl
    from scarplet_amd import _lib, _plan, segments
    from scarplet_amd.core import _context
    z = pr.synthetic_z(a.n)
    rng = np.random.default_rng(1)
    cells = rng.integers(0, z.size, a.cells)
    ang = 0.2 + 0.1 * rng.standard_normal(a.cells)
    lab = np.arange(a.cells) // a.segment + 1
    ages = _plan.age_grid()
    m = sl.Matcher(sl.DEMGrid.from_array(z, 1.0))      # the DEM on the device: the routes without an upload
    ctx = _context(0)
    M = a.width
    args = segments.check_args(z.shape, 1.0, cells, lab, ang, float(a.half), float(a.swath), ages, 1.0, 20, 1)
    segments.check_park(args, M)
    seg = lambda ramp: segments._run(ctx, args, z.shape[1], False, False, ramp=ramp)
    prof = lambda **kw: m.fit_profiles(cells, float(a.half), float(a.swath), angle=ang, min_samples=20, **kw)
    runs = {"fit_segments": lambda: seg(None),
            "fit_profiles, max_width": lambda: prof(max_width=float(M)),
            "fit_profiles, initial_slope": lambda: prof(max_width=float(M), initial_slope=a.slope),
            "fit_segments, max_width": lambda: seg((M, _lib.RAMP_FREE, 0.0)),
            "fit_segments, initial_slope": lambda: seg((M, _lib.RAMP_SLOPE, a.slope)),
            "fit_segments, max_width=0": lambda: seg((0, _lib.RAMP_FREE, 0.0))}
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
        print("%-30s k_profile device time %.2f ms (median of %d, warm; min %.2f, max %.2f); wall %.2f ms (min %.2f, max %.2f); %d of %d rows fitted"
              % (name, dev_ms[name], a.reps, min(dev), max(dev), 1e3 * float(np.median(wall)), 1e3 * min(wall), 1e3 * max(wall), int((out["status"] != 1).sum()),
                 len(out)), flush=True)
        if "width_index" in out.dtype.names:
            fit = out["status"] != 1
            print("%-30s width_index: mean %.2f, at the end of the range (status 8) in %d rows"
                  % ("", float(out["width_index"][fit].mean()), int((out["status"][fit] & 8 != 0).sum())))
    h, A, K = a.half, len(ages), a.cells
    per = 8 * ((2 * h + 1) + 4 * A * (M + 1))
    print("%d cells of %d x %d in %d segments of %d, h %d, w %d, %d ages, M %d: %d (m, age) pairs a cell (%d rounds of 64 lanes)"
          % (K, a.n, a.n, lab[-1], a.segment, h, a.swath, A, M, A * (M + 1), -(-A * (M + 1) // 64)))
    print("parked between the passes: %.2f GB of profiles and %.2f GB of per-pair terms, %d bytes a cell: %d chunks of at most "
          "%d cells" % (K * (2 * h + 1) * 8 / 1e9, K * 4 * A * (M + 1) * 8 / 1e9, per, -(-K * per // _lib.SEGMENT_MAX_PARK),
                        _lib.SEGMENT_MAX_PARK // per))
    for mode in ("max_width", "initial_slope"):
        print("fit_segments, %s / fit_profiles, %s, device time: %.2f (budget: at most 2)"
              % (mode, mode, dev_ms["fit_segments, " + mode] / dev_ms["fit_profiles, " + mode]))
    print("fit_segments, max_width=0 / fit_segments, device time: %.2f"
          % (dev_ms["fit_segments, max_width=0"] / dev_ms["fit_segments"]))
    assert _lib.K_NAMES[_lib.K_PROFILE] == "k_profile"


if __name__ == "__main__":
    main()
