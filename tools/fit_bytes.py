#!/usr/bin/env python3
"""Developer check: the bytes of sl.fit_profiles and sl.fit_segments, with and without max_shift, as SHA-256 lines.

Every case of the GPU tests (profile_reference.gpu_cases(), the profile and segment lists of shift_reference,
segment_reference.gpu_cases()) goes through every call it has the inputs for, with every optional output requested:
the unshifted call, the shifted call at the case's D (--shift cells where the case names none, cut to h - min_samples)
and the shifted call at D = 0.  One line per (case, call, output).  Two libraries that compute the same thing print the
same lines: run it once per library (SCARPLET_HIP_LIB selects one) and diff.  The hashes depend on the device's erf and
are not fixtures."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shift", type=int, default=2)
ap.add_argument("--small", action="store_true", help="without h1024 and the million cells of profile_reference")
a = ap.parse_args()


def main():
    import profile_reference as pr
    import segment_reference as sr
    import shift_reference as sh
    import scarplet_amd as sl
    from scarplet_amd import _lib
    print("# build id %s" % _lib.load().sc_build_id().decode(), flush=True)

    def emit(listname, case, call, names, arrays):
        for name, arr in zip(names, arrays if isinstance(arrays, tuple) else (arrays,)):
            arr = np.ascontiguousarray(arr)
            print("%s | %s | %s | %s %s %s" % (listname, case["name"], call, name, arr.shape,
                                               hashlib.sha256(arr.tobytes()).hexdigest()), flush=True)

    lists = (("profile_reference", pr.gpu_cases(big=not a.small)), ("shift_reference profiles", sh.profile_cases()),
             ("shift_reference segments", sh.segment_cases()), ("segment_reference", sr.gpu_cases()))
    for listname, cases in lists:
        for case in cases:
            h, w, de = case["h"], case["w"], case["de"]
            g = sl.DEMGrid.from_array(case["z"], float(de))
            D = case.get("D", min(a.shift, h - case["min_samples"]))
            kw = dict(ages=case["ages"], delta=case["delta"], min_samples=case["min_samples"])
            ranges = (("", None), (" D=%d" % D, D), (" D=0", 0))
            for tag, d in ranges:
                shifted = d is not None
                skw = dict(max_shift=d * de, return_shift=True) if shifted else {}
                out = sl.fit_profiles(g, case["cells"], case["angle"], h * de, w * de, return_curve=True, **kw, **skw)
                emit(listname, case, "fit_profiles" + tag, ("table", "curve", "shift"), out)
                if "labels" in case:
                    out = sl.fit_segments(g, case["cells"], case["labels"], case["angle"], h * de, w * de,
                                          min_profiles=case.get("min_profiles", 1), return_cells=True, return_curve=True,
                                          **kw, **skw)
                    emit(listname, case, "fit_segments" + tag, ("table", "cells", "curve", "shift"), out)


if __name__ == "__main__":
    main()
