#!/usr/bin/env python3
"""Developer timing: weights and robust fits of sl.fit_segments (sc_fit_segments_robust) against
sl.fit_profiles(..., robust=...) (sc_fit_profiles_robust) on the same 10^6 cells of synthetic_scarp(4096) in 2000 segments
at h = 100, w = 5, 35 ages, T = 8, for both losses and once with a weight plane, and against the plain sl.fit_segments, in
the same run.

All calls run on the DEM a Matcher holds on the device; the library's k_profile bracket (HIP events around every kernel of
every chunk, every call sampled) is read around each call, warm, median of --reps.  The budget of docs/segments.md is the
ratio of the device times: the joint call at most twice the single fits."""
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
ap.add_argument("--iterations", type=int, default=8)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()


def main():
    import profile_reference as pr
    import scarplet_amd as sl
    from scarplet_amd import _lib, _plan, profiles, segments
    from scarplet_amd.core import _context
    z = pr.synthetic_z(a.n)
    rng = np.random.default_rng(1)
    cells = rng.integers(0, z.size, a.cells)
    ang = 0.2 + 0.1 * rng.standard_normal(a.cells)
    lab = np.arange(a.cells) // a.segment + 1
    ages = _plan.age_grid()
    plane = rng.uniform(0.5, 1.5, z.shape)
    m = sl.Matcher(sl.DEMGrid.from_array(z, 1.0))      # the DEM on the device: the routes without an upload
    ctx = _context(0)
    T = a.iterations
    args = segments.check_args(z.shape, 1.0, cells, lab, ang, float(a.half), float(a.swath), ages, 1.0, 20, 1)

    def seg(**kw):
        rb = segments.check_robust(z.shape, args, kw.get("weights"), kw.get("robust"), None, T, None, None, None)
        return segments._run(ctx, args, z.shape[1], False, False, robust=rb)

    prof = lambda **kw: m.fit_profiles(cells, float(a.half), float(a.swath), angle=ang, min_samples=20, iterations=T, **kw)
    runs = {"fit_segments": lambda: seg()}
    for loss in ("huber", "tukey"):
        runs["fit_profiles, %s" % loss] = lambda loss=loss: prof(robust=loss)
        runs["fit_segments, %s" % loss] = lambda loss=loss: seg(robust=loss)
    runs["fit_profiles, tukey, weights"] = lambda: prof(robust="tukey", weights=plane)
    runs["fit_segments, tukey, weights"] = lambda: seg(robust="tukey", weights=plane)
    runs["fit_segments, weights alone"] = lambda: seg(weights=plane)
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
              % (name, dev_ms[name], a.reps, min(dev), max(dev), 1e3 * float(np.median(wall)), 1e3 * min(wall), 1e3 * max(wall), int((out["status"] & 1 == 0).sum()),
                 len(out)), flush=True)
        if "n_dormant" in out.dtype.names:
            fit = out["status"] & 1 == 0
            print("%-30s n_dormant: %d profiles in %d rows; status 16 in %d rows; n_down %.1f %% of the points"
                  % ("", int(out["n_dormant"].sum()), int((out["n_dormant"] > 0).sum()), int((out["status"] & 16 != 0).sum()),
                     100.0 * out["n_down"][fit].sum() / max(1, out["n"][fit].sum())))
    h, A, K = a.half, len(ages), a.cells
    print("%d cells of %d x %d in %d segments of %d, h %d, w %d, %d ages, T %d" % (K, a.n, a.n, lab[-1], a.segment, h, a.swath, A, T))
    for wt in (False, True):
        per = 8 * ((2 * h + 1) * (2 if wt else 1) + _lib.SEGMENT_ROBUST_PLANES * A)
        print("parked %s a plane: %.2f GB of profiles%s and %.2f GB of per-age terms, %d bytes a cell: %d chunks of at most %d cells"
              % ("with" if wt else "without", K * (2 * h + 1) * 8 / 1e9, " and as much of weights" if wt else "",
                 K * _lib.SEGMENT_ROBUST_PLANES * A * 8 / 1e9, per, -(-K * per // _lib.SEGMENT_MAX_PARK),
                 _lib.segment_robust_cap(h, A, wt)))
    for mode in ("huber", "tukey", "tukey, weights"):
        print("fit_segments, %s / fit_profiles, %s, device time: %.2f (budget: at most 2)"
              % (mode, mode, dev_ms["fit_segments, " + mode] / dev_ms["fit_profiles, " + mode]))
    print("fit_segments, weights alone / fit_segments, device time: %.2f" % (dev_ms["fit_segments, weights alone"] / dev_ms["fit_segments"]))
    assert _lib.K_NAMES[_lib.K_PROFILE] == "k_profile" and profiles.ROBUST_LOSSES["huber"][0] == _lib.ROBUST_HUBER


if __name__ == "__main__":
    main()
