#!/usr/bin/env python3
"""Developer timing: sl.fit_profiles on 10^6 cells of synthetic_scarp(4096) at h = 100, w = 5, 35 ages.

The library's k_profile bracket (HIP events around the table kernel and the fit kernel of every chunk of cells, every
call sampled), warm, median of --reps; the wall clock of the call beside it; the model's gathered bytes and FP64
operations; and the numpy restatement (tests/profile_reference.py) on a seeded sample of 2000 of the cells, spread
over the cores this process may use, for scale.  The model is a count, not a measurement: per cell (2w + 1)(2h + 1)
bilinear samples of four float64 each, and per cell and age four passes over 2h + 1 points of about 4, 7, 8 and 6
operations."""
import argparse
import multiprocessing as mp
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
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--sample", type=int, default=2000)
ap.add_argument("--no-reference", action="store_true")
a = ap.parse_args()


def _restate(job):
    import profile_reference as pr
    n, cells, ang, h, w, ages = job
    z = pr.synthetic_z(n)                              # (regenerated in the worker: cheaper than pickling 134 MB)
    return len(pr.fit_profiles(z, 1.0, cells, ang, h, w, ages, min_samples=20))


def main():
    import profile_reference as pr
    from scarplet_amd import _lib, _plan
    z = pr.synthetic_z(a.n)
    rng = np.random.default_rng(1)
    cells = rng.integers(0, z.size, a.cells)
    ang = 0.2 + 0.1 * rng.standard_normal(a.cells)
    ages = _plan.age_grid()
    ref_s = None
    if not a.no_reference:
        # the pool runs before this process opens the device
        pick = np.sort(np.random.default_rng(5).choice(a.cells, min(a.sample, a.cells), replace=False))
        ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        ncpu = max(1, min(ncpu, 16))
        jobs = [(a.n, cells[p], ang[p], a.half, a.swath, ages) for p in np.array_split(pick, ncpu)]
        t = time.perf_counter()
        with mp.get_context("spawn").Pool(ncpu) as pool:
            done = sum(pool.map(_restate, jobs))
        ref_s = time.perf_counter() - t
        assert done == len(pick)

    import scarplet_amd as sl
    from scarplet_amd.core import _context
    g = sl.DEMGrid.from_array(z, 1.0)
    m = sl.Matcher(g)                                  # the DEM on the device: the route without an upload
    ctx = _context(0)
    run = lambda: m.fit_profiles(cells, float(a.half), float(a.swath), angle=ang, min_samples=20)
    out = run()                                        # warm-up (buffers sized)
    wall, dev = [], []
    for _ in range(a.reps):
        ctx.profile(1)
        ms0 = ctx.profile_get()["k_profile"][1]
        t = time.perf_counter()
        run()
        wall.append(time.perf_counter() - t)
        dev.append(ctx.profile_get()["k_profile"][1] - ms0)
        ctx.profile(0)
    dev_ms, wall_ms = float(np.median(dev)), 1e3 * float(np.median(wall))
    h, w, A, K = a.half, a.swath, len(ages), a.cells
    np_ = 2 * h + 1
    gathered = K * (2 * w + 1) * np_ * 4 * 8.0
    flops = K * ((2 * w + 1) * np_ * 20.0 + A * np_ * (4 + 7 + 8 + 6.0))
    fitted = int((out["status"] != 1).sum())
    print("%d cells of %d x %d, h %d, w %d, %d ages: %d fitted" % (K, a.n, a.n, h, w, A, fitted))
    print("k_profile device time %.2f ms (median of %d, warm; min %.2f, max %.2f); wall %.1f ms"
          % (dev_ms, a.reps, min(dev), max(dev), wall_ms))
    print("model: %.1f GB gathered (%.1f TB/s of cache traffic at that time), %.1f GFLOP FP64 (%.1f TFLOP/s)"
          % (gathered / 1e9, gathered / 1e12 / (dev_ms * 1e-3), flops / 1e9, flops / 1e12 / (dev_ms * 1e-3)))
    print("%.2f us per cell, %.1f ns per cell and age" % (1e3 * dev_ms / K, 1e6 * dev_ms / K / A))
    if ref_s is not None:
        print("numpy restatement: %d cells in %.1f s on %d cores = %.2f ms per cell and core; the device's %d cells "
              "would take it %.0f s" % (len(pick), ref_s, ncpu, 1e3 * ref_s * ncpu / len(pick), K, ref_s * K / len(pick)))
    assert _lib.K_NAMES[_lib.K_PROFILE] == "k_profile"


if __name__ == "__main__":
    main()
