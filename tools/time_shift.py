#!/usr/bin/env python3
"""Developer timing: the centre shift (max_shift) of sl.fit_profiles and sl.fit_segments against the unshifted calls on
the same 10^6 cells of synthetic_scarp(4096) at h = 100, w = 5, 35 ages, D = 8 cells, in the same run.

The cells and segments are those of tools/time_segments.py (2000 segments of 500).  All four calls go through a Matcher
that holds the DEM on the device; the library's k_profile bracket (HIP events around every kernel of every chunk, every
call sampled) is read around each call, warm, median of --reps.  The budget of docs/profiles.md is the ratio of the
device times: at most 2 D + 1 = 17, the independent fits the search replaces."""
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
ap.add_argument("--shift", type=int, default=8)
ap.add_argument("--reps", type=int, default=10)
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
    D = a.shift
    args = segments.check_args(z.shape, 1.0, cells, lab, ang, float(a.half), float(a.swath), ages, 1.0, 20, 1)
    sargs = segments.check_args(z.shape, 1.0, cells, lab, ang, float(a.half), float(a.swath), ages, 1.0, 20, 1, shift=True)
    prof = lambda **kw: m.fit_profiles(cells, float(a.half), float(a.swath), angle=ang, min_samples=20, **kw)
    runs = {"fit_profiles": lambda: prof(),
            "fit_profiles, max_shift": lambda: prof(max_shift=float(D)),
            "fit_segments": lambda: segments._run(ctx, args, z.shape[1], False, False),
            "fit_segments, max_shift": lambda: segments._run(ctx, sargs, z.shape[1], False, False, shift=D)}
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
        print("%-26s k_profile device time %.2f ms (median of %d, warm; min %.2f, max %.2f); wall %.1f ms; %d of %d rows fitted"
              % (name, dev_ms[name], a.reps, min(dev), max(dev), 1e3 * float(np.median(wall)), int((out["status"] != 1).sum()),
                 len(out)), flush=True)
        if "shift_index" in out.dtype.names:
            fit = out["status"] != 1
            print("%-26s |shift_index|: mean %.2f, at the end of the range (status 8) in %d rows"
                  % ("", float(np.abs(out["shift_index"][fit]).mean()), int((out["status"][fit] & 8 != 0).sum())))
    h, A, K = a.half, len(ages), a.cells
    print("%d cells of %d x %d in %d segments of %d, h %d, w %d, %d ages, D %d: %d (age, shift) pairs a cell, %d rounds of 64 lanes"
          % (K, a.n, a.n, lab[-1], a.segment, h, a.swath, A, D, A * (2 * D + 1), -(-A * (2 * D + 1) // 64)))
    print("erf table %.1f KB; parked between the passes of fit_segments: %.2f GB of profiles, %.2f GB of per-age terms, %.3f GB of shifts"
          % ((2 * (h + D) + 1) * A * 8 / 1e3, K * (2 * h + 1) * 8 / 1e9, K * 4 * A * 8 / 1e9, K * A / 1e9))
    for base in ("fit_profiles", "fit_segments"):
        print("%s with max_shift / without, device time: %.2f (budget: at most 2 D + 1 = %d)"
              % (base, dev_ms[base + ", max_shift"] / dev_ms[base], 2 * D + 1))
    assert _lib.K_NAMES[_lib.K_PROFILE] == "k_profile"


if __name__ == "__main__":
    main()
