#!/usr/bin/env python3
"""Developer timing: the weights and robust fits of sl.fit_profiles (docs/profiles.md, "Weights and robust fits") against
the plain call, on the same cells in the same run.

10^6 random cells of synthetic_scarp(4096) at h = 100, w = 5, 35 ages, T = --iterations, through the matcher that holds
the DEM.  Every line is the library's k_profile bracket (HIP events around the table kernel and the fit kernel of every
chunk), warm, median of --reps, beside the wall clock of the call, and its ratio to the plain call's.  By sweep count
the robust call makes (3 T + 5) / 4 of the plain call's sweeps; the budget is twice that.  The split: the same call at
T = 1 gives the cost of an iterate, the same call with the scale given leaves the order statistic out, and the weight
plane's lines show what the second sample per point and the LDS reads of u cost."""
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
ap.add_argument("--iterations", type=int, default=8)
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()


def main():
    import profile_reference as pr
    import scarplet_amd as sl
    from scarplet_amd.core import _context
    z = pr.synthetic_z(a.n)
    rng = np.random.default_rng(1)
    cells = rng.integers(0, z.size, a.cells)
    ang = 0.2 + 0.1 * rng.standard_normal(a.cells)
    plane = rng.uniform(0.2, 3.0, z.shape)
    m = sl.Matcher(sl.DEMGrid.from_array(z, 1.0))      # the DEM on the device: the route without an upload
    ctx = _context(0)
    T = a.iterations

    def timed(**kw):
        run = lambda: m.fit_profiles(cells, float(a.half), float(a.swath), angle=ang, min_samples=20, **kw)
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
        return out, float(np.median(dev)), min(dev), max(dev), 1e3 * float(np.median(wall))

    print("%d cells of %d x %d, h %d, w %d, 35 ages, T = %d; k_profile device time, median of %d, warm"
          % (a.cells, a.n, a.n, a.half, a.swath, T, a.reps))
    lines = [("plain", {}, 4),
             ("huber", dict(robust="huber", iterations=T), 3 * T + 5),
             ("tukey", dict(robust="tukey", iterations=T), 3 * T + 5),
             ("huber, T = 1", dict(robust="huber", iterations=1), 8),
             ("huber, scale given", dict(robust="huber", iterations=T, robust_scale=0.05), 3 * T + 5),
             ("weights alone", dict(weights=plane), 4),
             ("weights and huber", dict(weights=plane, robust="huber", iterations=T), 3 * T + 5)]
    ms = {}
    for name, kw, sweeps in lines:
        out, dev, lo, hi, wall = timed(**kw)
        ms[name] = dev
        fitted = int(((out["status"] & 1) == 0).sum())
        extra = ""
        if "robust" in kw:
            extra = "; %d rows moved off the least squares age, median n_down %d" % (
                int((out["kt_index"] != out["ls_index"]).sum()), int(np.median(out["n_down"])))
        print("%-20s %8.2f ms (min %.2f, max %.2f); wall %7.1f ms; %2d sweeps, %5.2f x them; %5.2f x plain; %d fitted%s"
              % (name, dev, lo, hi, wall, sweeps, sweeps / 4.0, dev / ms["plain"], fitted, extra))
    ratio = (3 * T + 5) / 4.0
    for name in ("huber", "tukey"):
        r = ms[name] / ms["plain"]
        print("%s: %.2f x the plain call; by sweep count %.2f x, the budget %.2f x: %s"
              % (name, r, ratio, 2 * ratio, "inside" if r <= 2 * ratio else "MISSED"))
    if T > 1:
        it = (ms["huber"] - ms["huber, T = 1"]) / (T - 1)
        print("split (huber): an iterate of three sweeps %.2f ms = %.2f x a plain sweep; the order statistic %.2f ms; "
              "iterate 0, the scale and the loss sweep %.2f ms"
              % (it, it / 3 / (ms["plain"] / 4), ms["huber"] - ms["huber, scale given"], ms["huber, T = 1"] - it))


if __name__ == "__main__":
    main()
