#!/usr/bin/env python3
"""Developer timing: sl.extract_traces on the benchmark plan's result (synthetic_scarp(10000), Scarp, scale 100).

Both routes, wall clock after a warm-up, median of --reps: Matcher.extract_traces (sc_trace_result: the planes formed
and traced on the device) and sl.extract_traces (sc_trace_planes: the 3.2 GB of planes uploaded first, then traced);
the upload alone (one hipMemcpy of the planes into a device buffer of their size); the library's
k_trace bracket (device time of the trace kernels, every call sampled); K; and the numpy / scipy reference
(tests/trace_reference.py) on the same box.  The floor it is set against is a model, not a measurement: about
30 bytes per cell (snr and angle read once, the u8 mask, int32 parent and label traffic) at 5 TB/s."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import scarplet_amd as sl  # noqa: E402
from scarplet_amd import _lib, _plan, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--ages", type=int, default=35, help="ages of the search (the benchmark plan: 35)")
ap.add_argument("--no-reference", action="store_true")
a = ap.parse_args()

m = sl.Matcher(synthetic.synthetic_scarp(a.n))
t0 = time.time()
res = np.array(m.search(sl.Scarp, 100., _plan.age_grid()[:a.ages], _plan.angle_grid()).result_array())
print("search %dx%d x %d ages x 181: %.2f s" % (a.n, a.n, a.ages, time.time() - t0), flush=True)
smax = np.nanmax(res[3])
lo, hi, mc = 0.2 * smax, 0.5 * smax, 20
print("snr_low %.6g snr_high %.6g min_cells %d" % (lo, hi, mc))
ctx = m.ctx
planes = np.ascontiguousarray(res)


def timed(fn):
    fn()                                           # warm-up (buffers sized, pages touched)
    wall, dev = [], []
    for _ in range(a.reps):
        ctx.profile(1)
        n0, ms0 = ctx.profile_get()["k_trace"]
        t = time.perf_counter()
        out = fn()
        wall.append(time.perf_counter() - t)
        n1, ms1 = ctx.profile_get()["k_trace"]
        dev.append(ms1 - ms0)
        ctx.profile(0)
    return out, 1e3 * float(np.median(wall)), float(np.median(dev))


out_r, wall_r, dev_r = timed(lambda: m.extract_traces(lo, hi, mc))
out_p, wall_p, dev_p = timed(lambda: ctx.trace_planes(planes, lo, hi, mc))
K = len(out_r.segments)
assert K == len(out_p[2]) and np.array_equal(out_r.labels, out_p[1])

# the upload alone: the same host-to-device copy into a device buffer of the same size, through the HIP runtime the
# library itself links (no second GPU framework in the process)
import ctypes  # noqa: E402
try:
    hip = ctypes.CDLL("libamdhip64.so")
except OSError:
    hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
dptr = ctypes.c_void_p()
assert hip.hipMalloc(ctypes.byref(dptr), ctypes.c_size_t(planes.nbytes)) == 0
src = planes.ctypes.data_as(ctypes.c_void_p)
up = []
for rep in range(a.reps + 1):
    t = time.perf_counter()
    assert hip.hipMemcpy(dptr, src, ctypes.c_size_t(planes.nbytes), 1) == 0      # hipMemcpyHostToDevice
    assert hip.hipDeviceSynchronize() == 0
    if rep:
        up.append(time.perf_counter() - t)
upload = 1e3 * float(np.median(up))
assert hip.hipFree(dptr) == 0

cells = float(a.n) * a.n
floor_ms = 30.0 * cells / 5e12 * 1e3
print("K %d segments, %d segment cells, %d thinned cells" % (K, int((out_r.labels > 0).sum()), int(out_r.thin.sum())))
print("Matcher.extract_traces (sc_trace_result): wall %.1f ms (median of %d), k_trace device %.2f ms"
      % (wall_r, a.reps, dev_r))
print("sl.extract_traces route (sc_trace_planes): wall %.1f ms, k_trace device %.2f ms" % (wall_p, dev_p))
print("upload of the planes (%.2f GB, pageable host memory): %.1f ms = %.1f GB/s"
      % (planes.nbytes / 1e9, upload, planes.nbytes / 1e9 / (upload * 1e-3)))
print("floor model: 30 B/cell at 5 TB/s = %.2f ms; device time / floor = %.2f (sc_trace_result) - the floor is %.2f "
      "of the measured device time" % (floor_ms, dev_r / floor_ms, floor_ms / dev_r))
if not a.no_reference:
    import trace_reference as tr
    t = time.perf_counter()
    tr.trace(res, lo, hi, mc)
    print("numpy / scipy reference (tests/trace_reference.py): %.2f s" % (time.perf_counter() - t))
assert _lib.K_NAMES[_lib.K_TRACE] == "k_trace"
