#!/usr/bin/env python3
"""Developer timing and coverage of sl.bootstrap_segments (docs/bootstrap.md).

Timing (the default): the 10^6 cells in 2000 segments of tools/time_segments.py - synthetic_scarp(4096), h = 100, w = 5,
35 ages - at R = 1000 with blocks of 10 cells, against sc_fit_segments on the same cells in the same run.  Both go
through the context that holds the DEM; the library's k_profile bracket is read around each call, warm, median of
--reps.  The budget is the ratio of the two device times: at most 2.  The kernel split is taken by difference: the same
call at R = 1 (stage one, the block terms and next to no replicates) against R = 1000.

--coverage N: over N noise seeds of synthetic_scarp(600, sigma=0.5, theta=0.2) and the 100 cells of docs/segments.md
(h = 100, w = 2, blocks of 30: about ten cells each), how often the level = 0.95 interval of the bootstrap holds the true
index 10, and how often fit_segments' [lo_index, hi_index] does.  --cpu runs the coverage on the numpy restatement
(tests/bootstrap_reference.py) without a device; fit_segments' interval is then walked along sse_i = Spp - Q_i of the
same terms."""
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
ap.add_argument("--block", type=int, default=10)
ap.add_argument("--half", type=int, default=100)
ap.add_argument("--swath", type=int, default=5)
ap.add_argument("--replicates", type=int, default=1000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--coverage", type=int, default=0)
ap.add_argument("--cpu", action="store_true")
a = ap.parse_args()


def timing():
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
    # blocks of --block consecutive cells of each segment, handed over as CSR (random cells have no strike to cut along)
    idx, sa, ca, seg_start, seg_label = sargs.cells, sargs.sa, sargs.ca, sargs.seg_start, sargs.seg_label
    blk_start = np.unique(np.concatenate([np.arange(s0, s1, a.block) for s0, s1 in zip(seg_start[:-1], seg_start[1:])]
                                         + [[len(idx)]])).astype(np.int64)
    seg_blk_start = np.searchsorted(blk_start[:-1], seg_start).astype(np.int64)

    def boot(R):
        return ctx.bootstrap_segments(idx, sa, ca, seg_start, seg_label, seg_blk_start, blk_start, sargs.ages, a.half, a.swath, 0, 1.0,
                                      20, 1, 5, R, 0.95, 0)[0]
    runs = {"fit_segments": lambda: segments._run(ctx, sargs, z.shape[1], False, False),
            "bootstrap_segments R = %d" % a.replicates: lambda: boot(a.replicates),
            "bootstrap_segments R = 1": lambda: boot(1)}
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
        print("%-32s k_profile device time %.2f ms (median of %d, warm; min %.2f, max %.2f); wall %.2f ms (min %.2f, max %.2f); %d of %d rows done"
              % (name, dev_ms[name], a.reps, min(dev), max(dev), 1e3 * float(np.median(wall)), 1e3 * min(wall), 1e3 * max(wall), int((out["status"] != 1).sum()),
                 len(out)))
    full, one = dev_ms["bootstrap_segments R = %d" % a.replicates], dev_ms["bootstrap_segments R = 1"]
    print("%d cells of %d x %d in %d segments of %d, blocks of %d cells (%d blocks), h %d, w %d, %d ages"
          % (a.cells, a.n, a.n, lab[-1], a.segment, a.block, len(blk_start) - 1, a.half, a.swath, len(ages)))
    print("kernel split by difference: stage one, block terms and summary (the R = 1 call) %.2f ms; the replicates %.2f ms"
          % (one, full - one))
    ratio = full / dev_ms["fit_segments"]
    print("bootstrap_segments / fit_segments device time: %.2f (budget: at most 2)%s"
          % (ratio, "" if ratio <= 2 else " - MISSED, see the split above"))


def coverage():
    import bootstrap_reference as br
    import profile_reference as pr
    import segment_reference as sr
    from scarplet_amd import _plan
    ages = _plan.age_grid()
    _, cells, theta = sr.noisy_case()
    lab = np.ones(len(cells), dtype=int)
    inside = {"bootstrap": 0, "fit_segments": 0}
    width = {"bootstrap": 0, "fit_segments": 0}
    if not a.cpu:
        import scarplet_amd as sl
    for k in range(a.coverage):
        z = pr.synthetic_z(600, sigma=0.5, theta=theta, seed=1000 + k)
        if a.cpu:
            row = br.bootstrap_segments(z, 1.0, cells, lab, theta, 100, 2, ages, 30.0, 1000, seed=k)[0]
            blo, bhi = row["lo_index"], row["hi_index"]
            # fit_segments' interval from the same terms: sse_i = Spp - Q_i, dof = n - 2 n_profiles - 1
            T = row["terms"].sum(axis=0)
            n, spp = 0, 0.0
            for c in cells:
                p, j, nn, ok = br.sh.profile_of(z, c, np.sin(theta), np.cos(theta), 100, 2, 4)
                s = j.astype(np.float64)
                Q = np.linalg.qr(np.stack([np.ones_like(s), s], axis=1))[0]
                p2 = p - Q @ (Q.T @ p)
                n, spp = n + nn, spp + float(p2 @ p2)
            best, flo, fhi, _ = pr.choose(spp - T[:, 1] ** 2 / T[:, 0], n - 2 * len(cells) - 1 + 3, 1.0)
        else:
            g = sl.DEMGrid.from_array(z, 1.0)
            row = sl.bootstrap_segments(g, cells, lab, theta, 100., 2., block_length=30., seed=k)[0]
            fit = sl.fit_segments(g, cells, lab, theta, 100., 2.)[0]
            blo, bhi, flo, fhi = row["lo_index"], row["hi_index"], fit["lo_index"], fit["hi_index"]
        inside["bootstrap"] += int(blo <= 10 <= bhi)
        inside["fit_segments"] += int(flo <= 10 <= fhi)
        width["bootstrap"] += int(bhi - blo + 1)
        width["fit_segments"] += int(fhi - flo + 1)
    print("coverage over %d noise seeds (%s): synthetic_scarp(600, sigma=0.5, theta=0.2, seed=1000..), 100 cells, h 100, w 2, "
          "blocks of 30, R 1000, level 0.95" % (a.coverage, "the numpy restatement" if a.cpu else "the device"))
    for name in ("bootstrap", "fit_segments"):
        print("%-14s interval holds the true index 10 in %d of %d (%.1f %%); mean width %.2f grid steps"
              % (name, inside[name], a.coverage, 100.0 * inside[name] / a.coverage, width[name] / a.coverage))


if __name__ == "__main__":
    coverage() if a.coverage else timing()
