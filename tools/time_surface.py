#!/usr/bin/env python3
"""Developer timing of sl.snr_surface (docs/surface.md).

The workload: synthetic_scarp(4096), Scarp at scale 100, the default 35 ages x 181 orientations, the cells of
extract_traces on that search.

The yardstick is the only other route to the same numbers: after the search, ctx.score_cells_f64(cells[:256], n_t) - a
workgroup per (cell, template) over whole boxes - against snr_surface(..., return_surface=True) on the same 256 cells, both
returning the full cubes, warm, wall time, median of --reps.  The new call must take less time; the ratio is printed.

Then the new call alone at --cells cells: device time under the library's k_settle bracket and wall time, warm, median of
--reps.  --split first runs that call in a child process under `rocprofv3 --kernel-trace --stats` and prints the time of k_sf_score
and k_sf_reduce per launch (a run of its own: the profiler's numbers are not mixed with the timings below)."""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--scale", type=float, default=100.0)
ap.add_argument("--cells", type=int, default=10000)
ap.add_argument("--old-cells", type=int, default=256)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--split", action="store_true", help="also: the kernels' shares from a rocprofv3 run of a child process")
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
a = ap.parse_args()


def median_ms(run, reps):
    run()                                              # warm-up (buffers sized)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), 1e3 * min(t), 1e3 * max(t)


def main():
    import scarplet_amd as sl
    from scarplet_amd import _lib, _plan, synthetic
    ages, angles = _plan.age_grid(), _plan.angle_grid()
    n_t = len(ages) * len(angles)
    m = sl.Matcher(synthetic.synthetic_scarp(a.n))
    t0 = time.perf_counter()
    m.search(sl.Scarp, a.scale, ages, angles)
    res = m.result_array()
    print("search of %d x %d, Scarp at scale %g, %d x %d templates: %.2f s" % (a.n, a.n, a.scale, len(ages), len(angles),
                                                                              time.perf_counter() - t0))
    snr = res[3]
    tr = m.extract_traces(float(np.percentile(snr[snr > 0], 99.0)))
    cells = np.flatnonzero(tr.labels.ravel() > 0)
    print("extract_traces at the 99th percentile of the SNR: %d cells in %d segments" % (len(cells), len(tr.segments)))
    if len(cells) < a.cells:
        raise SystemExit("the trace has %d cells, fewer than --cells %d" % (len(cells), a.cells))
    surf = lambda c: m.snr_surface(sl.Scarp, a.scale, ages, angles, c, return_surface=True)
    if a.child:                                        # (under the profiler: the one call whose kernels are wanted)
        surf(cells[:a.cells])
        surf(cells[:a.cells])
        return
    few = cells[:a.old_cells]
    rc = np.column_stack([few // a.n, few % a.n]).astype(np.int32)
    # the old route first: it needs the search's tables in the context, the new call replaces them
    old = median_ms(lambda: m.ctx.score_cells_f64(rc, n_t), a.reps)
    o_amp, o_snr = m.ctx.score_cells_f64(rc, n_t)
    new = median_ms(lambda: surf(few), a.reps)
    tab, S, Amp = surf(few)
    o_snr = o_snr.reshape(len(few), len(angles), len(ages)).transpose(0, 2, 1)
    err = float((np.abs(S - o_snr).max(axis=0) / np.maximum(o_snr.max(axis=0), 1e-300)).max())
    print("%d cells x %d templates, full cubes, wall, warm, median of %d:" % (len(few), n_t, a.reps))
    print("  score_cells_f64 (a workgroup per pair, whole boxes)   %9.1f ms (min %.1f, max %.1f)" % old)
    print("  snr_surface(return_surface=True)                      %9.1f ms (min %.1f, max %.1f)" % new)
    print("  old / new: %.1f (the new call must take less time)%s; largest difference of the two cubes %.1e of a "
          "template's largest SNR" % (old[0] / new[0], "" if new[0] < old[0] else " - MISSED", err))
    many = cells[:a.cells]
    surf(many)
    wall, dev = [], []
    for _ in range(a.reps):
        m.ctx.profile(1)
        ms0 = m.ctx.profile_get()["k_settle"][1]
        t0 = time.perf_counter()
        out = surf(many)
        wall.append(time.perf_counter() - t0)
        dev.append(m.ctx.profile_get()["k_settle"][1] - ms0)
        m.ctx.profile(0)
    t0 = time.perf_counter()
    m.snr_surface(sl.Scarp, a.scale, ages, angles, many)
    rows_only = time.perf_counter() - t0
    print("snr_surface at %d cells (%.1e pairs): k_settle device time %.1f ms (median of %d, warm; min %.1f, max %.1f); wall "
          "%.1f ms with the cubes (2 x %.0f MB copied out), %.1f ms the rows alone; %d of %d cells live"
          % (len(many), float(len(many)) * n_t, float(np.median(dev)), a.reps, min(dev), max(dev), 1e3 * float(np.median(wall)),
             8e-6 * len(many) * n_t, 1e3 * rows_only, int((out[0]["status"] != 1).sum()), len(many)))
    print("k_sf_score: %d cells a workgroup, a thread per (age, cell), a stage of 512 taps a cell (rows per group = 512 / the "
          "orientation's widest row span, at least 1), 64 ages a pass" % _lib.SURFACE_CELL_BATCH)


def split():
    prof = shutil.which("rocprofv3")
    if not prof:
        print("kernel split: no rocprofv3 on this machine")
        return
    d = tempfile.mkdtemp(prefix="time_surface_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--child", "--n", str(a.n), "--scale", str(a.scale), "--cells", str(a.cells)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            print("kernel split: the profiler run failed (%d)\n%s" % (r.returncode, r.stderr[-2000:]))
            return
        rows = {row["Name"].split("(")[0].replace("void ", ""): row for row in csv.DictReader(open(files[0]))}
        sc, rd = rows.get("k_sf_score"), rows.get("k_sf_reduce")
        if not sc or not rd:
            print("kernel split: the kernels are not in the trace: %s" % sorted(rows)[:20])
            return
        f = lambda row: (int(row["Calls"]), float(row["TotalDurationNs"]) / 1e6 / int(row["Calls"]))
        print("kernel split (rocprofv3 --kernel-trace --stats, a run of its own): k_sf_score %d launches of %.2f ms, k_sf_reduce "
              "%d launches of %.3f ms" % (f(sc) + f(rd)))
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    if a.split and not a.child:
        split()                                        # (first: the child is started by a process that has not opened the device)
    main()
