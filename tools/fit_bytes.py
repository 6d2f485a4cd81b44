#!/usr/bin/env python3
"""Developer check: the bytes of every call of the fit family through the public API - sl.fit_profiles and sl.fit_segments with
and without max_shift, with max_width in both modes, with weights and a robust loss and with refine, sl.bootstrap_segments,
sl.fit_along_strike and sl.lateral_offsets - as SHA-256 lines.

Every case of the GPU tests (profile_reference.gpu_cases(), the profile and segment lists of shift_reference,
segment_reference.gpu_cases()) goes through every call it has the inputs for, with every optional output requested:
the unshifted call, the shifted call at the case's D (--shift cells where the case names none, cut to h - min_samples)
and the shifted call at D = 0.  The other segment calls take the case lists of their own reference modules
(segment_ramp_reference, segment_robust_reference for Huber and Tukey, segment_refine_reference at refine 0, 1 and 2,
bootstrap_reference, strike_reference), and so do the other profile calls (robust_reference for Huber and Tukey,
ramp_reference with the width free and with the slope given, refine_reference at refine 0, 1 and 2) and sl.lateral_offsets
(the DEMs, stations and parameters of tests/test_gpu_lateral.py, made by lateral_reference).  One line
per (case, call, output), the output hashed raw, and a last line with the totals and the launches counted.  --fit-chunk N sets option "fit_chunk"
on the context the calls share, so that most cases run in several chunks (64 does that for these lists).  Two libraries
that compute the same thing print the same lines: run it once per library (SCARPLET_HIP_LIB selects one) and diff.  The
hashes depend on the device's erf and are not fixtures."""
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
ap.add_argument("--fit-chunk", type=int, default=0, help='option "fit_chunk": the cells at which a driver closes a chunk')
ap.add_argument("--segments-only", action="store_true", help="the segment calls alone: no fit_profiles")
a = ap.parse_args()


def main():
    import bootstrap_reference as br
    import profile_reference as pr
    import ramp_reference as rx
    import refine_reference as rf
    import robust_reference as rr
    import segment_refine_reference as sf
    import segment_ramp_reference as sx
    import segment_reference as sr
    import segment_robust_reference as qr
    import shift_reference as sh
    import strike_reference as stk
    import test_gpu_lateral as tl
    import scarplet_amd as sl
    from scarplet_amd import _lib, core
    # (to stderr: the build id is what differs between two libraries that print the same lines)
    print("# build id %s, fit_chunk %d" % (_lib.load().sc_build_id().decode(), a.fit_chunk), file=sys.stderr, flush=True)
    ctx = core._context(0)
    ctx.set_option("fit_chunk", a.fit_chunk)
    ctx.profile(0)                                       # (the launch counters from zero)
    total = dict(calls=0, buffers=0, bytes=0)

    def emit(listname, case, call, names, arrays):
        total["calls"] += 1
        for name, arr in zip(names, arrays if isinstance(arrays, tuple) else (arrays,)):
            arr = np.ascontiguousarray(arr)
            total["buffers"] += 1
            total["bytes"] += arr.nbytes
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
                if not a.segments_only:
                    out = sl.fit_profiles(g, case["cells"], case["angle"], h * de, w * de, return_curve=True, **kw, **skw)
                    emit(listname, case, "fit_profiles" + tag, ("table", "curve", "shift"), out)
                if "labels" in case:
                    out = sl.fit_segments(g, case["cells"], case["labels"], case["angle"], h * de, w * de,
                                          min_profiles=case.get("min_profiles", 1), return_cells=True, return_curve=True,
                                          **kw, **skw)
                    emit(listname, case, "fit_segments" + tag, ("table", "cells", "curve", "shift"), out)

    def profiles(c, **kw):
        return sl.fit_profiles(sl.DEMGrid.from_array(c["z"], float(c["de"])), c["cells"], c["angle"], c["h"] * c["de"],
                               c["w"] * c["de"], ages=c["ages"], delta=c["delta"], min_samples=c["min_samples"], return_curve=True,
                               **kw)

    if not a.segments_only:
        for loss in ("huber", "tukey"):
            for name, c in rr.gpu_cases(loss).items():
                emit("robust_reference " + loss, dict(name=name), "fit_profiles robust", ("table", "curve"),
                     profiles(c, weights=c["weights"], **c["robust"]))
        for c in rx.gpu_cases():
            for tag, slope in (("free", None),) + ((("slope", c["slope"]),) if c["slope"] is not None else ()):
                out = profiles(c, max_width=c["M"] * c["de"], initial_slope=slope, return_width=True)
                emit("ramp_reference", c, "fit_profiles max_width " + tag, ("table", "curve", "width"), out)
        for c in rf.gpu_cases():
            if a.small and c["name"] == "h1024":
                continue
            for R in (0, 1, 2):
                emit("refine_reference", c, "fit_profiles refine=%d" % R, ("table", "curve"), profiles(c, refine=R))
        for name in tl.DEMS:
            z, de = tl.dem(name)
            cells, ang = tl.stations(name, 257)
            for p in tl.PARAMS:
                h, D, q0, q1, ms = p
                out = sl.lateral_offsets(sl.DEMGrid.from_array(z, de), cells, ang, h * de, q0 * de, q1 * de, D * de, min_samples=ms,
                                         return_curve=True)
                emit("lateral_reference", dict(name="%s h%d D%d q%d..%d" % ((name,) + p[:4])), "lateral_offsets",
                     ("table", "curve"), out)

    def segments(c, **kw):
        return sl.fit_segments(sl.DEMGrid.from_array(c["z"], float(c["de"])), c["cells"], c["labels"], c["angle"], c["h"] * c["de"],
                               c["w"] * c["de"], ages=c["ages"], delta=c["delta"], min_samples=c["min_samples"],
                               min_profiles=c.get("min_profiles", 1), return_cells=True, return_curve=True, **kw)

    for c in sx.gpu_cases():
        for tag, slope in (("free", None), ("slope", c["slope"])):
            out = segments(c, max_width=c["M"] * c["de"], initial_slope=slope, return_width=True)
            emit("segment_ramp_reference", c, "fit_segments max_width " + tag, ("table", "cells", "curve", "width"), out)
    for loss in ("huber", "tukey"):
        for name, c in qr.gpu_cases(loss).items():
            out = segments(c, weights=c["weights"], **c["robust"])
            emit("segment_robust_reference " + loss, dict(name=name), "fit_segments robust", ("table", "cells", "curve"), out)
    for c in sf.gpu_cases():
        for R in (0, 1, 2):
            emit("segment_refine_reference", c, "fit_segments refine=%d" % R, ("table", "cells", "curve"), segments(c, refine=R))
    for c in br.gpu_cases():
        out = sl.bootstrap_segments(sl.DEMGrid.from_array(c["z"], 1.0), c["cells"], c["labels"], c["angle"], float(br.H), float(br.W),
                                    block_length=c["block_length"], replicates=c["R"], seed=c["seed"], ages=c["ages"],
                                    min_samples=c["min_samples"], min_blocks=c["min_blocks"],
                                    max_shift=float(c["D"]) if c["D"] else None, return_hist=True, return_replicates=True)
        emit("bootstrap_reference", c, "bootstrap_segments", ("table", "hist", "index", "amplitude"), out)
    for c in stk.gpu_cases():
        out = sl.fit_along_strike(sl.DEMGrid.from_array(c["z"], 1.0), c["cells"], c["labels"], c["angle"], float(c["h"]), float(c["w"]),
                                  window=c["window"], step=c["step"], ages=c["ages"], delta=c["delta"], min_samples=c["min_samples"],
                                  min_profiles=c["min_profiles"], max_shift=float(c["D"]) if c["D"] else None, return_curve=True)
        emit("strike_reference", c, "fit_along_strike", ("table", "curve"), out)
    # (the launches show that the chunks ran: the same for two libraries, more with --fit-chunk)
    print("# %d calls, %d buffers, %d bytes, %d launches under k_profile"
          % (total["calls"], total["buffers"], total["bytes"], ctx.profile_get()["k_profile"][0]), flush=True)


if __name__ == "__main__":
    main()
