#!/opt/conda/bin/python3.9
"""Golden fixture of CalculationMixin._estimate_curvature_noiselevel (dem.py:152-179).

Runs where the reference and the Anaconda interpreter are (like oracle/gen_golden.py, whose
import_reference() it uses):

    /opt/conda/bin/python3.9 tools/gen_noiselevel_golden.py

Calls the UNMODIFIED reference method on four grids and writes tests/golden/ref_noiselevel.npz:
slices of the existing DEM fixtures (not copies of them), the cells set to NaN, the cell sizes
and the reference's (angles, mean, sd).  Case "tiny" is a seeded 9 x 13 random grid, stored as
it is (the filter radius, 400, is many times its size: the reflections repeat).  About a minute.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from gen_golden import import_reference, ref_grid  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")

# name: (fixture, rows, cols, dx, dy, NaN cells as (r0, r1, c0, c1) boxes)
CASES = {
    "gc": ("dem_grandcanyon.npz", (0, 512), (0, 480), 2.0, 2.0, [(5, 7, 5, 8)]),
    "carrizo": ("dem_carrizo.npz", (300, 600), (100, 360), 2.0, 2.0, []),
    "gc_dy": ("dem_grandcanyon.npz", (120, 420), (200, 480), 1.0, -1.0, []),
}


def case_grid(name):
    fx, (r0, r1), (c0, c1), dx, dy, nans = CASES[name]
    z = np.load(os.path.join(GOLDEN, fx))["z"][r0:r1, c0:c1].astype(float)
    for a, b, c, d in nans:
        z[a:b, c:d] = np.nan
    return z, dx, dy


def tiny_grid():
    rng = np.random.default_rng(2024)
    z = np.cumsum(rng.standard_normal((9, 13)), axis=1) + 0.3 * rng.standard_normal((9, 13))
    z[4, 6] = np.nan
    return z, 1.5, 1.5


def main():
    _, dem, _ = import_reference()
    out = {}
    grids = {k: case_grid(k) for k in CASES}
    grids["tiny"] = tiny_grid()
    for name, (z, dx, dy) in grids.items():
        g = ref_grid(dem, z, dx, dy)
        t = time.time()
        angles, mean, sd = g._estimate_curvature_noiselevel()
        print("%-8s %s dx %g dy %g: %.1f s, angle 0: mean %r sd %r" % (name, z.shape, dx, dy, time.time() - t,
                                                                       mean[0], sd[0]), flush=True)
        assert np.array_equal(np.isnan(g._griddata), np.zeros(z.shape, bool))      # the write-through
        out[name + "_angles"] = np.asarray(angles)
        out[name + "_mean"] = np.asarray(mean, dtype=np.float64)
        out[name + "_sd"] = np.asarray(sd, dtype=np.float64)
        out[name + "_d"] = np.array([dx, dy])
        if name == "tiny":
            out["tiny_z"] = z
        else:
            fx, rows, cols, _, _, nans = CASES[name]
            out[name + "_fixture"] = np.array(fx)
            out[name + "_slice"] = np.array(rows + cols)
            out[name + "_nan_boxes"] = np.array(nans, dtype=np.int64).reshape(-1, 4)
    np.savez_compressed(os.path.join(GOLDEN, "ref_noiselevel.npz"), **out)
    print("wrote tests/golden/ref_noiselevel.npz")


if __name__ == "__main__":
    main()
