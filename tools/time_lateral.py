#!/usr/bin/env python3
"""Developer timing of sl.lateral_offsets (docs/lateral.md).

--stations random cells of synthetic_scarp(--n) with strikes about 0.2, h = --half, the band --near..--far, D = --lag:
the call goes through the context that holds the DEM; the library's k_profile bracket is read around it, warm, median of
--reps, beside the wall time of the whole call, and both are turned into (station, lag, point) visits a second - a visit
is one point of one lag of one station, which the kernel touches in each of its three passes.  A second line has
D = --small-lag, where 2 D + 1 < 64 leaves lanes idle; two more show the stages almost alone (D = 0; one line a side).
The numpy restatement (tests/lateral_reference.py) is timed first, on --ref-stations of the same stations spread over
--procs processes - forked before this process touches the device - and scaled to all of them."""
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
ap.add_argument("--stations", type=int, default=10 ** 5)
ap.add_argument("--half", type=int, default=200)
ap.add_argument("--near", type=int, default=5)
ap.add_argument("--far", type=int, default=20)
ap.add_argument("--lag", type=int, default=50)
ap.add_argument("--small-lag", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--procs", type=int, default=16)
ap.add_argument("--ref-stations", type=int, default=320)
a = ap.parse_args()

Z = None


def _restate(job):
    import lateral_reference as lr
    cells, ang, D = job
    t = time.perf_counter()
    rows = lr.lateral_offsets(Z, 1.0, cells, ang, a.half, a.near, a.far, D)[0]
    return time.perf_counter() - t, rows


def restatement(cells, ang, D):
    """(seconds for all the stations on a.procs processes, scaled from a.ref_stations of them; their rows)."""
    import multiprocessing as mp
    m = min(a.ref_stations, len(cells))
    parts = [(cells[i:m:a.procs], ang[i:m:a.procs], D) for i in range(a.procs)]
    with mp.get_context("fork").Pool(a.procs) as pool:
        pool.map(_restate, [(cells[:1], ang[:1], D)] * a.procs)          # (warm: imports)
        t = time.perf_counter()
        out = pool.map(_restate, parts)
        wall = time.perf_counter() - t
    rows = np.concatenate([r for _, r in out])
    order = np.concatenate([np.arange(i, m, a.procs) for i in range(a.procs)])
    back = np.empty(m, dtype=np.int64)
    back[order] = np.arange(m)
    return wall * len(cells) / m, rows[back]


def main():
    global Z
    import profile_reference as pr
    Z = pr.synthetic_z(a.n)
    rng = np.random.default_rng(1)
    cells = rng.integers(0, Z.size, a.stations)
    ang = 0.2 + 0.1 * rng.standard_normal(a.stations)
    ref_s, ref_rows = restatement(cells, ang, a.lag)

    import scarplet_amd as sl
    from scarplet_amd import lateral
    from scarplet_amd.core import _context
    sl.Matcher(sl.DEMGrid.from_array(Z, 1.0))           # the DEM on the device: the route without an upload
    ctx = _context(0)
    print("%d stations of %d x %d, h %d, band %d..%d" % (a.stations, a.n, a.n, a.half, a.near, a.far))
    dev_s = {}
    # the two budget lines, then the stages almost alone: no lags but 0 (sampling and one pass over u and v), and a band of
    # one line a side (a sixteenth of the samples at the defaults) under all the lags
    for D, near, what in ((a.lag, a.near, ""), (a.small_lag, a.near, ""), (0, a.near, " [stage 1 almost alone]"),
                          (a.lag, a.far, " [band %d..%d: stage 2 almost alone]" % (a.far, a.far))):
        args = lateral.check_args(Z.shape, 1.0, cells, ang, float(a.half), float(near), float(a.far), float(D), 1.0, 8)
        run = lambda: lateral._run(ctx, args, Z.shape[1], False)
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
        visits = float(a.stations) * (2 * D + 1) * (2 * a.half + 1)
        dev_s[(D, near)] = 1e-3 * float(np.median(dev))
        samples = float(a.stations) * (4 * a.half + 2 * D + 2) * (a.far - near + 1)
        print("D %3d%s (%3d lags, %d rounds of 64 lanes): k_profile device time %.2f ms (median of %d, warm; min %.2f, max %.2f); "
              "wall %.1f ms; %.3g visits: %.3g visits/s on the device, %.3g by the wall; %.3g bilinear samples; %d of %d fitted"
              % (D, what, 2 * D + 1, (2 * D + 64) // 64, 1e3 * dev_s[(D, near)], a.reps, min(dev), max(dev), 1e3 * float(np.median(wall)),
                 visits, visits / dev_s[(D, near)], visits / float(np.median(wall)), samples, int((out["status"] != 1).sum()), len(out)))
        if D == a.lag and near == a.near:
            m = len(ref_rows)
            same = all(np.array_equal(out[f][:m], ref_rows[f]) for f in ("n", "lag", "lo", "hi", "status"))
            close = all(np.allclose(out[f][:m], ref_rows[f], rtol=1e-9, atol=0, equal_nan=True)
                        for f in ("offset", "mse", "rho", "dz", "tilt"))
            print("      the restatement on %d processes: %.1f s for these stations (scaled from %d of them): %.0f x the device "
                  "time, %.0f x the wall; its rows %s the device's"
                  % (a.procs, ref_s, m, ref_s / dev_s[(D, near)], ref_s / float(np.median(wall)),
                     "equal" if same and close else "DIFFER FROM"))
    print("idle lanes: D %d has %.2f of the visits of D %d and takes %.2f of its device time"
          % (a.small_lag, (2 * a.small_lag + 1) / float(2 * a.lag + 1), a.lag, dev_s[(a.small_lag, a.near)] / dev_s[(a.lag, a.near)]))


if __name__ == "__main__":
    main()
