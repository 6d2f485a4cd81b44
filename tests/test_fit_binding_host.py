"""The fit family's binding without a device: a Context built by ``Context.__new__`` around a library that records
``(name, args)`` drives each of the eleven wrappers of scarplet_amd/_lib.py in every form - plain, _dem, shifted, each
optional output on and off - and so reaches all 26 symbols.  Every recorded call must fit its SIGNATURES entry, argument for
argument, and the outputs must have the documented shapes and dtypes.  ``replay`` renders the same calls as text
(tools/fit_binding_dump.py prints it for two trees to compare)."""
import ctypes as C
import itertools

import numpy as np

from scarplet_amd import _lib

K, A, S, NB, NW, R = 3, 2, 2, 3, 2, 4
F64, I8, I32 = np.dtype(np.float64), np.dtype(np.int8), np.dtype(np.int32)


class FakeLib(object):
    """Stands for libscarplet_hip.so: every function records its name and arguments and returns SC_OK."""

    def __init__(self):
        self.log = []

    def sc_destroy(self, h):
        pass

    def __getattr__(self, name):
        def call(h, *args):
            self.log.append((name, h, args))
            return _lib.SC_OK
        return call


def fake_context():
    ctx = _lib.Context.__new__(_lib.Context)
    ctx.lib = FakeLib()
    ctx._h = C.c_void_p(1)
    return ctx


def inputs():
    return dict(cells=np.array([5, 7, 9], dtype=np.int64), sa=np.array([0.0, 0.6, 0.8]), ca=np.array([1.0, 0.8, 0.6]),
                seg_start=np.array([0, 2, 3], dtype=np.int64), seg_label=np.array([1, 2], dtype=np.int32),
                ages=np.array([1.0, 2.0]), seg_blk_start=np.array([0, 2, 3], dtype=np.int64),
                blk_start=np.array([0, 1, 2, 3], dtype=np.int64), seg_win_start=np.array([0, 1, 2], dtype=np.int64),
                win_lo=np.array([0, 2], dtype=np.int64), win_hi=np.array([2, 3], dtype=np.int64),
                z=np.arange(20.0).reshape(4, 5), weights=np.ones((4, 5)))


def forms(x):
    """(method, positional arguments, keywords, symbol, outputs) of every wrapper and form; ``outputs``: per item of the
    return tuple the flag that asks for it (None: always there), its shape and its dtype."""
    P = (x["cells"], x["sa"], x["ca"], x["ages"], 4, 1, 1.5, 1.0, 2)
    G = (x["cells"], x["sa"], x["ca"], x["seg_start"], x["seg_label"], x["ages"], 4, 1, 1.5, 1.0, 2, 1)
    rob = dict(loss=_lib.ROBUST_HUBER, tuning=1.345, iterations=3, scale=0.5)
    L = _lib
    return [
        ("fit_profiles", P, {}, "sc_fit_profiles", [(None, (K,), L.PROFILE_DTYPE), ("curve", (K, A), F64)]),
        ("fit_profiles", P, dict(shift=1), "sc_fit_profiles_shift",
         [(None, (K,), L.PROFILE_SHIFT_DTYPE), ("curve", (K, A), F64), ("shift_plane", (K, A), I8)]),
        ("fit_profiles_robust", P, rob, "sc_fit_profiles_robust", [(None, (K,), L.PROFILE_ROBUST_DTYPE), ("curve", (K, A), F64)]),
        ("fit_profiles_robust", P, dict(rob, weights=x["weights"]), "sc_fit_profiles_robust",
         [(None, (K,), L.PROFILE_ROBUST_DTYPE), ("curve", (K, A), F64)]),
        ("fit_profiles_ramp", P + (2,), dict(mode=L.RAMP_SLOPE, slope=0.6), "sc_fit_profiles_ramp",
         [(None, (K,), L.PROFILE_RAMP_DTYPE), ("curve", (K, A), F64), ("width_plane", (K, A), I8)]),
        ("fit_profiles_refine", P + (2,), {}, "sc_fit_profiles_refine", [(None, (K,), L.PROFILE_FINE_DTYPE), ("curve", (K, A), F64)]),
        ("fit_segments", G, {}, "sc_fit_segments",
         [(None, (S,), L.SEGMENT_FIT_DTYPE), ("cell_table", (K,), L.SEGMENT_CELL_DTYPE), ("curve", (S, A), F64)]),
        ("fit_segments", G, dict(shift=1), "sc_fit_segments_shift",
         [(None, (S,), L.SEGMENT_FIT_DTYPE), ("cell_table", (K,), L.SEGMENT_SHIFT_CELL_DTYPE), ("curve", (S, A), F64),
          ("shift_plane", (K, A), I8)]),
        ("fit_segments_ramp", G + (2,), dict(mode=L.RAMP_SLOPE, slope=0.6), "sc_fit_segments_ramp",
         [(None, (S,), L.SEGMENT_RAMP_FIT_DTYPE), ("cell_table", (K,), L.SEGMENT_CELL_DTYPE), ("curve", (S, A), F64),
          ("width_plane", (S, A), I8)]),
        ("fit_segments_robust", G, rob, "sc_fit_segments_robust",
         [(None, (S,), L.SEGMENT_ROBUST_FIT_DTYPE), ("cell_table", (K,), L.SEGMENT_ROBUST_CELL_DTYPE), ("curve", (S, A), F64)]),
        ("fit_segments_robust", G, dict(rob, weights=x["weights"]), "sc_fit_segments_robust",
         [(None, (S,), L.SEGMENT_ROBUST_FIT_DTYPE), ("cell_table", (K,), L.SEGMENT_ROBUST_CELL_DTYPE), ("curve", (S, A), F64)]),
        ("fit_segments_refine", G + (1,), {}, "sc_fit_segments_refine",
         [(None, (S,), L.SEGMENT_FINE_FIT_DTYPE), ("cell_table", (K,), L.SEGMENT_FINE_CELL_DTYPE), ("curve", (S, A), F64)]),
        ("bootstrap_segments", (x["cells"], x["sa"], x["ca"], x["seg_start"], x["seg_label"], x["seg_blk_start"], x["blk_start"],
                                x["ages"], 4, 1, 1, 1.5, 2, 1, 2, R, 0.9, 2 ** 63 + 5), {}, "sc_bootstrap_segments",
         [(None, (S,), L.SEGMENT_BOOT_DTYPE), ("hist", (S, A), I32), ("replicates", (S, R + 1), I8),
          ("replicates", (S, R + 1), F64)]),
        ("fit_strike", (x["cells"], x["sa"], x["ca"], x["seg_start"], x["seg_label"], x["seg_win_start"], x["win_lo"], x["win_hi"],
                        x["ages"], 4, 1, 1, 1.5, 1.0, 2, 1), {}, "sc_fit_strike",
         [(None, (NW,), L.STRIKE_FIT_DTYPE), ("curve", (NW, A), F64)]),
        ("lateral_offsets", (x["cells"], x["sa"], x["ca"], 4, 1, 3, 2, 1.5, 1.0, 3), {}, "sc_lateral_offsets",
         [(None, (K,), L.LATERAL_FIT_DTYPE), ("curve", (K, 5), F64)]),
    ]


def drive(x):
    """Every form of ``forms`` through a fake context, on the context's DEM and on ``z``, each optional output on and
    off: yields (symbol expected, the recorded call, the outputs, the outputs expected as (shape, dtype) or None)."""
    ctx = fake_context()
    for method, pos, kw, symbol, outputs in forms(x):
        flags = sorted({f for f, _, _ in outputs if f is not None})
        for z in (None, x["z"]):
            for on in itertools.product((False, True), repeat=len(flags)):
                asked = dict(zip(flags, on))
                got = getattr(ctx, method)(*pos, z=z, **kw, **asked)
                want = [(shape, dt) if f is None or asked[f] else None for f, shape, dt in outputs]
                yield symbol + ("_dem" if z is not None else ""), ctx.lib.log[-1], got, want


def test_every_wrapper_and_form_fits_its_signature():
    seen = set()
    for symbol, (name, h, args), got, want in drive(inputs()):
        assert name == symbol
        seen.add(name)
        argtypes = _lib.SIGNATURES[name][1]
        assert isinstance(h, C.c_void_p) and argtypes[0] is C.c_void_p
        assert len(args) + 1 == len(argtypes), name
        for i, a in enumerate(args):
            argtypes[i + 1].from_param(a)                # (raises where ctypes would refuse the argument)
            # (from_param lets an int pass for a double and any pointer for a void*: the stricter half)
            if argtypes[i + 1] is C.c_double:
                assert isinstance(a, float), (name, i, a)
            elif argtypes[i + 1] in (C.c_int, C.c_longlong, C.c_uint64):
                assert isinstance(a, int) and not isinstance(a, bool), (name, i, a)
            else:
                assert a is None or isinstance(a, argtypes[i + 1]), (name, i, a)
        assert len(got) == len(want)
        for arr, w in zip(got, want):
            if w is None:
                assert arr is None
            else:
                assert isinstance(arr, np.ndarray) and arr.shape == w[0] and arr.dtype == w[1] and arr.flags.c_contiguous
    fit = {n for n in _lib.SIGNATURES if n.startswith(("sc_fit_", "sc_bootstrap_", "sc_lateral_"))}
    assert len(fit) == 26 and seen == fit


def replay():
    """The calls of ``drive`` as text, one line each: the symbol, then every argument - a number as it is, a pointer as its
    ctypes type and the array it points to (an input by name, an output by its place in the return tuple)."""
    x = inputs()
    lines = []
    for symbol, (name, h, args), got, want in drive(x):
        where = {v.ctypes.data: k for k, v in x.items()}
        where.update({arr.ctypes.data: "out%d%s%s" % (i, arr.shape, arr.dtype.str if arr.dtype.names is None else "rows")
                      for i, arr in enumerate(got) if arr is not None and arr.size})
        shown = []
        for a in args:
            if a is None or isinstance(a, (int, float)):
                shown.append(repr(a))
            else:
                shown.append("%s:%s" % (type(a).__name__, where.get(C.cast(a, C.c_void_p).value, "?")))
        lines.append("%s(%s)" % (name, ", ".join(shown)))
    return lines
