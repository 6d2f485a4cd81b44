#!/usr/bin/env python3
"""Developer timing: sl.fit_segments against sl.fit_profiles on the same 10^6 cells of synthetic_scarp(4096) at
h = 100, w = 5, 35 ages, in the same run.

The cells are those of tools/time_profiles.py; consecutive runs of them form the segments (--segment cells each, the
last one shorter).  Both calls go through a Matcher that holds the DEM on the device; the library's k_profile bracket
(HIP events around every kernel of every chunk, every call sampled) is read around each call, warm, median of --reps.
The budget of docs/segments.md is the ratio of the two device times: at most 2."""
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
ap.add_argument("--reps", type=int, default=20)
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
    args = segments.check_args(z.shape, 1.0, cells, lab, ang, float(a.half), float(a.swath), ages, 1.0, 20, 1)
    runs = {"fit_profiles": lambda: m.fit_profiles(cells, float(a.half), float(a.swath), angle=ang, min_samples=20),
            "fit_segments": lambda: segments._run(ctx, args, z.shape[1], False, False),
            "fit_segments, cell table and curves": lambda: segments._run(ctx, args, z.shape[1], True, True)}
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
        first = out[0] if isinstance(out, tuple) else out
        print("%-36s k_profile device time %.2f ms (median of %d, warm; min %.2f, max %.2f); wall %.2f ms (min %.2f, max %.2f); %d of %d rows fitted"
              % (name, dev_ms[name], a.reps, min(dev), max(dev), 1e3 * float(np.median(wall)), 1e3 * min(wall), 1e3 * max(wall), int((first["status"] != 1).sum()),
                 len(first)))
    h, A, K = a.half, len(ages), a.cells
    print("%d cells of %d x %d in %d segments of %d, h %d, w %d, %d ages" % (K, a.n, a.n, lab[-1], a.segment, h, a.swath, A))
    print("parked between the passes: %.2f GB of profiles and %.2f GB of per-age terms"
          % (K * (2 * h + 1) * 8 / 1e9, K * 4 * A * 8 / 1e9))
    print("fit_segments / fit_profiles device time: %.2f (budget: at most 2)"
          % (dev_ms["fit_segments"] / dev_ms["fit_profiles"]))
    assert _lib.K_NAMES[_lib.K_PROFILE] == "k_profile"


if __name__ == "__main__":
    main()
