"""sl.snr_surface on the CPU: argument validation before the library is loaded, the table's fields, the layout of
sc_surface_row and the header's ABI, the exported symbol, the kernels' scratch, the numpy restatement
(tests/surface_reference.py) on hand-made cubes, and the ground the GPU comparisons stand on, asserted on the oracle alone."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import surface_reference as ref
from scarplet_amd import _lib, surface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- every argument error is a ValueError before the library is loaded -------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    import scarplet_amd.core as core

    def refuse(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(core, "_context", refuse)
    monkeypatch.setattr(_lib, "load", refuse)


def test_arguments_validate_before_the_library_is_loaded(no_library):
    import scarplet_amd as sl
    g = sl.DEMGrid.from_array(np.zeros((40, 50)), 2.0)
    holed = np.zeros((40, 50))
    holed[3, 4] = np.nan
    ok = dict(data=g, Template=sl.Scarp, cells=[3, 77, 3], scale=10)
    bad = [
        (dict(drop=1.0), "drop = 1"),
        (dict(drop=-0.1), "drop < 0"),
        (dict(drop=np.nan), "drop NaN"),
        (dict(drop=np.inf), "drop inf"),
        (dict(drop="much"), "drop not a number"),
        (dict(drop=True), "drop a bool"),
        (dict(ages=[]), "no age"),
        (dict(angles=[]), "no orientation"),
        (dict(ages=[1.0, np.nan]), "age NaN"),
        (dict(angles=[[0.0, 0.1]]), "angles 2-D"),
        (dict(ages=np.arange(1, 258.0), angles=np.linspace(-1, 1, 256)), "257 x 256 = 65792 templates"),
        (dict(cells=[3, 2000]), "a cell outside the DEM"),
        (dict(cells=[-1]), "a negative cell"),
        (dict(cells=([1, 2], [3, 50])), "a column outside the DEM"),
        (dict(cells=[0.5]), "cells not integers"),
        (dict(cells=np.zeros((4, 5), dtype=bool)), "a bool plane of another shape"),
        (dict(data=sl.DEMGrid.from_array(holed, 2.0)), "a DEM with a NaN cell"),
        (dict(data=np.zeros((40, 50))), "data not a DEMGrid"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError):
            sl.snr_surface(**dict(ok, **kw))
            pytest.fail(what)
    with pytest.raises(ValueError, match="fill"):
        sl.snr_surface(**dict(ok, data=sl.DEMGrid.from_array(holed, 2.0)))
    with pytest.raises(TypeError):
        sl.snr_surface(**dict(ok, Template=sl.Crater))
    # what is valid gets as far as the device
    for kw in (dict(), dict(drop=0), dict(drop=0.999), dict(ages=[3.0], angles=[0.2]), dict(cells=([1, 2], [3, 49])),
               dict(ages=np.arange(1, 256.0), angles=np.linspace(-1, 1, 257)), dict(return_surface=True)):
        with pytest.raises(AssertionError, match="the library was asked for"):
            sl.snr_surface(**dict(ok, **kw))
    idx, par, ang, keep = surface.check_args((40, 50), [3, 77, 3], None, None, 0.1)
    assert idx.tolist() == [3, 77, 3] and len(par) == 35 and len(ang) == 181 and keep == 1.0 - 0.1


def test_more_cells_than_the_library_takes(monkeypatch):
    assert surface.MAX_CELLS == 2 ** 31 - 1
    monkeypatch.setattr(surface, "MAX_CELLS", 2)                           # (not an array of 2^31 cells)
    with pytest.raises(ValueError, match="2\\^31"):
        surface.check_args((40, 50), [1, 2, 3], None, None, 0.1)
    surface.check_args((40, 50), [1, 2], None, None, 0.1)


def test_matcher_route_validates(no_library):
    import scarplet_amd as sl
    from scarplet_amd import dist, traces

    class Held(object):
        whole, nan_dem, ny, nx, de = True, False, 40, 50, 2.0

        def describe(self, *a, **k):
            raise AssertionError("the library was asked for")
    call = lambda m, cells=[3, 77], drop=0.1, par=[1.0, 2.0], ang=[0.0]: sl.Matcher.snr_surface(m, sl.Scarp, 10, par, ang, cells, drop=drop)
    part = Held()
    part.whole = False
    with pytest.raises(ValueError, match="block"):
        call(part)
    nan = Held()
    nan.nan_dem = True
    with pytest.raises(ValueError, match="fill"):
        call(nan)
    with pytest.raises(ValueError, match="DistMatcher"):
        dist.DistMatcher.snr_surface(object(), sl.Scarp, 10, [1.0], [0.0], [3])
    for kw in (dict(drop=1.0), dict(cells=[2000]), dict(par=[]), dict(ang=[]), dict(par=np.arange(1, 258.0), ang=np.linspace(-1, 1, 256))):
        with pytest.raises(ValueError):
            call(Held(), **kw)
    tr = traces.Traces(np.zeros((30, 50), dtype=bool), np.zeros((30, 50), dtype=np.int32),
                       traces._table(np.zeros(0, dtype=_lib.SEGMENT_DTYPE)))
    with pytest.raises(ValueError, match="shape"):
        call(Held(), tr)
    with pytest.raises(TypeError):
        sl.Matcher.snr_surface(Held(), sl.Crater, 10, [1.0], [0.0], [3])
    with pytest.raises(AssertionError, match="the library was asked for"):
        call(Held())
    # no cells: an empty table without a device call
    out = call(Held(), cells=[])
    assert len(out) == 0 and out.dtype == surface.DTYPE
    tr = traces.Traces(np.zeros((40, 50), dtype=bool), np.zeros((40, 50), dtype=np.int32),
                       traces._table(np.zeros(0, dtype=_lib.SEGMENT_DTYPE)))
    out, s, a = sl.Matcher.snr_surface(Held(), sl.Scarp, 10, [1.0, 2.0], [0.0, 0.1, 0.2], tr, return_surface=True)
    assert out.dtype.names[-1] == "label" and s.shape == (0, 2, 3) and a.shape == (0, 2, 3)


def test_table_fields():
    assert surface.DTYPE.names == ("row", "col", "cell", "par_index", "ang_index", "par", "angle", "amp", "snr", "par_lo_index",
                                   "par_hi_index", "par_lo", "par_hi", "ang_lo_index", "ang_hi_index", "angle_lo", "angle_hi",
                                   "n_within", "status")
    import scarplet_amd as sl
    assert sl.snr_surface is surface.snr_surface and hasattr(sl.Matcher, "snr_surface")
    rows = np.zeros(2, dtype=_lib.SURFACE_ROW_DTYPE)
    rows[0] = (1, 2, 0, 1, 2, 2, 5, 2 + 4 + 16, 7.5, -0.25)
    rows[1] = (-1, -1, -1, -1, -1, -1, 0, 1, np.nan, np.nan)
    par, ang = np.array([1.0, 10.0]), np.array([-0.5, 0.0, 0.5])
    t = surface.table(rows, np.array([57, 3]), 50, par, ang, label=np.array([4, 9]))
    assert t["row"].tolist() == [1, 0] and t["col"].tolist() == [7, 3] and t["cell"].tolist() == [57, 3]
    assert t[0]["par"] == 10.0 and t[0]["angle"] == 0.5 and t[0]["par_lo"] == 1.0 and t[0]["par_hi"] == 10.0
    assert t[0]["angle_lo"] == 0.5 and t[0]["angle_hi"] == 0.5 and t[0]["snr"] == 7.5 and t[0]["amp"] == -0.25
    assert t[0]["n_within"] == 5 and t[0]["status"] == 22 and t["label"].tolist() == [4, 9]
    assert all(np.isnan(t[1][f]) for f in ("par", "angle", "par_lo", "par_hi", "angle_lo", "angle_hi", "snr", "amp"))
    assert t[1]["par_index"] == -1 and t[1]["ang_hi_index"] == -1 and t[1]["status"] == 1


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_surface_row_layout_matches_c(tmp_path):
    S, dt = _lib.sc_surface_row, _lib.SURFACE_ROW_DTYPE
    names = [f for f, _ in S._fields_]
    body = '  printf("%zu\\n", sizeof(sc_surface_row));\n'
    body += "".join('  printf("%%zu\\n", offsetof(sc_surface_row, %s));\n' % f for f in names)
    prog = tmp_path / "surface.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarplet_hip.h"\nint main(void) {\n' + body
                    + '  printf("%d %d\\n", SC_K_COUNT, SC_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "surface"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert vals == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in names] + [11, 10]
    assert ctypes.sizeof(S) == 48 and dt.itemsize == 48 and dt.names == tuple(names)
    assert [dt.fields[f][1] for f in names] == [getattr(S, f).offset for f in names]
    assert names == ["par_index", "ang_index", "par_lo", "par_hi", "ang_lo", "ang_hi", "n_within", "status", "snr", "amp"]
    assert [f for f, _ in ref.ROW_FIELDS] == names
    assert len(_lib.K_NAMES) == 11 and _lib.ABI_VERSION == 10


def test_header_declares_the_call_and_keeps_the_abi():
    txt = open(os.path.join(ROOT, "include", "scarplet_hip.h")).read()
    assert "#define SC_ABI_VERSION 10\n" in txt
    assert re.search(r"#define\s+SC_K_COUNT\s+11\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint sc_snr_surface\s*\(", code)
    assert len(_lib.SIGNATURES["sc_snr_surface"][1]) == 10


def test_library_exports_the_call():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "sc_snr_surface") and "sc_snr_surface" in _lib.SIGNATURES
    assert _lib.load().sc_abi_version() == 10


def test_build_id_covers_the_new_source():
    mk = open(os.path.join(ROOT, "scarplet_amd", "csrc", "Makefile")).read()
    src = re.search(r"^SRC\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "sc_surface.hip" in src and re.search(r"^ID_SRC\s*=\s*\$\(SRC\) \$\(HDR\)$", mk, flags=re.M)
    hip = open(os.path.join(ROOT, "scarplet_amd", "csrc", "sc_surface.hip")).read()
    assert int(re.search(r"constexpr int SF_CB = (\d+);", hip).group(1)) == _lib.SURFACE_CELL_BATCH


def test_surface_kernels_use_no_scratch():
    from test_isa_budget import kernel_table
    t = kernel_table("sc_surface.hip")
    for k in ("k_sf_score", "k_sf_reduce"):
        assert k in t, sorted(t)
        assert t[k]["scratch"] == 0, (k, t[k])
    assert t["k_sf_score"]["vgpr"] + t["k_sf_score"]["agpr"] <= 128, t["k_sf_score"]      # four waves per SIMD
    # the preparation is the settle's, shared: one launch of k_st_sums / k_st_spans in the library, behind sc_window_runs
    src = {f: open(os.path.join(ROOT, "scarplet_amd", "csrc", f)).read() for f in ("sc_settle.hip", "sc_surface.hip")}
    assert src["sc_settle.hip"].count("hipLaunchKernelGGL(k_st_sums") == 1 and src["sc_settle.hip"].count("hipLaunchKernelGGL(k_st_spans") == 1
    assert "hipLaunchKernelGGL(k_st_" not in src["sc_surface.hip"]
    assert len(re.findall(r"\bsc_window_runs\(ctx, n, woff, wbuf", src["sc_settle.hip"] + src["sc_surface.hip"])) == 2


# ---- the restatement on hand-made cubes ------------------------------------------------------------------------------------
def one(S, drop=0.1, Amp=None):
    S = np.asarray(S, dtype=np.float64)[None]
    r = ref.reduce_cube(S, S * 0.5 if Amp is None else np.asarray(Amp, dtype=np.float64)[None], drop)[0]
    return {f: r[f].item() for f in r.dtype.names}


def test_restatement_ties_go_to_the_earlier_template():
    # S[ia, ib]; hand-over order t = ib * n_par + ia: (0,0) (1,0) (0,1) (1,1) (0,2) (1,2)
    r = one([[1.0, 5.0, 5.0], [5.0, 2.0, 3.0]])
    # 5.0 at (1,0) [t=1], (0,1) [t=2], (0,2) [t=4]: the first is t = 1
    assert (r["par_index"], r["ang_index"], r["snr"], r["amp"]) == (1, 0, 5.0, 2.5)
    # thr = 4.5: P = [5, 5], Q = [5, 5, 5]: both intervals cover their grids; three templates within
    assert (r["par_lo"], r["par_hi"], r["ang_lo"], r["ang_hi"], r["n_within"], r["status"]) == (0, 1, 0, 2, 3, 30)
    r = one([[7.0, 7.0]])                                                   # n_par = 1: orientation 0 before orientation 1
    assert (r["par_index"], r["ang_index"]) == (0, 0)
    r = one([[7.0], [7.0]])                                                 # n_ang = 1: age 0 before age 1
    assert (r["par_index"], r["ang_index"]) == (0, 0)


def test_restatement_counts_nan_as_minus_infinity():
    r = one([[np.nan, 2.0, np.nan], [1.0, np.nan, 1.9]], drop=0.1)
    assert (r["par_index"], r["ang_index"], r["snr"]) == (0, 1, 2.0)
    # thr = 1.8: P = [2, 1.9], Q = [1, 2, 1.9]
    assert (r["par_lo"], r["par_hi"], r["ang_lo"], r["ang_hi"], r["n_within"], r["status"]) == (0, 1, 1, 2, 2, 2 + 4 + 16)
    r = one([[np.nan, np.nan], [np.nan, np.nan]])
    assert r["status"] == 1 and r["par_index"] == -1 and r["n_within"] == 0 and np.isnan(r["snr"]) and np.isnan(r["amp"])
    r = one([[np.nan, 0.0], [-0.0, np.nan]])
    assert r["status"] == 1 and r["ang_hi"] == -1


def test_restatement_of_an_all_zero_cell():
    r = one(np.zeros((3, 4)))
    assert (r["par_index"], r["ang_index"], r["par_lo"], r["par_hi"], r["ang_lo"], r["ang_hi"]) == (-1,) * 6
    assert r["n_within"] == 0 and r["status"] == 1 and np.isnan(r["snr"]) and np.isnan(r["amp"])


def test_restatement_intervals_and_their_ends():
    # 5 ages x 6 orientations, a ridge: S = 10 - 2 |ia - 2| - |ib - 3|
    ia, ib = np.meshgrid(np.arange(5), np.arange(6), indexing="ij")
    S = 10.0 - 2.0 * np.abs(ia - 2) - np.abs(ib - 3)
    r = one(S, drop=0.1)                                                    # thr 9: P = 6 8 10 8 6, Q = 7 8 9 10 9 8
    assert (r["par_index"], r["ang_index"], r["par_lo"], r["par_hi"], r["ang_lo"], r["ang_hi"]) == (2, 3, 2, 2, 2, 4)
    assert r["n_within"] == 3 and r["status"] == 0
    r = one(S, drop=0.25)                                                   # thr 7.5: ages 1..3, orientations 1..5 (the last)
    assert (r["par_lo"], r["par_hi"], r["ang_lo"], r["ang_hi"], r["status"]) == (1, 3, 1, 5, 16)
    assert r["n_within"] == int((S >= 7.5).sum()) == 7
    r = one(S, drop=0.4)                                                    # thr 6: every age, every orientation
    assert (r["par_lo"], r["par_hi"], r["ang_lo"], r["ang_hi"], r["status"]) == (0, 4, 0, 5, 30)
    # each end on its own
    r = one(S[2:], drop=0.1)                                                # the best at the first age
    assert (r["par_index"], r["par_lo"], r["par_hi"], r["status"]) == (0, 0, 0, 2)
    r = one(S[:3], drop=0.1)
    assert (r["par_index"], r["par_lo"], r["par_hi"], r["status"]) == (2, 2, 2, 4)
    r = one(S[:, 3:], drop=0.05)                                            # thr 9.5: the best at the first orientation
    assert (r["ang_index"], r["ang_lo"], r["ang_hi"], r["status"]) == (0, 0, 0, 8)
    r = one(S[:, :4], drop=0.05)
    assert (r["ang_index"], r["ang_lo"], r["ang_hi"], r["status"]) == (3, 3, 3, 16)
    # the orientation interval does not wrap: a second ridge at the far end is not joined
    T = S.copy()
    T[2, 0] = 9.9
    r = one(T, drop=0.05)
    assert (r["ang_lo"], r["ang_hi"], r["n_within"], r["status"]) == (3, 3, 2, 0)
    # a walk stops at the first neighbour below the threshold, whatever lies beyond
    T = S.copy()
    T[4, 3] = 9.8
    r = one(T, drop=0.05)
    assert (r["par_lo"], r["par_hi"], r["n_within"]) == (2, 2, 2)


def test_restatement_of_degenerate_grids_and_drop_zero():
    r = one([[3.0, 4.0, 3.9]], drop=0.1)                                    # n_par = 1: thr 3.6
    assert (r["par_index"], r["par_lo"], r["par_hi"], r["ang_lo"], r["ang_hi"], r["status"]) == (0, 0, 0, 1, 2, 2 + 4 + 16)
    r = one([[3.0], [4.0], [3.9]], drop=0.1)                                # n_ang = 1
    assert (r["ang_index"], r["ang_lo"], r["ang_hi"], r["par_lo"], r["par_hi"], r["status"]) == (0, 0, 0, 1, 2, 8 + 16 + 4)
    r = one([[4.0]], drop=0.0)
    assert (r["n_within"], r["status"]) == (1, 30)
    # drop = 0: thr is the best itself - exact ties are within, nothing else
    r = one([[1.0, 5.0, 5.0, 4.999999], [5.0, 2.0, 3.0, 1.0]], drop=0.0)
    assert (r["par_index"], r["ang_index"], r["n_within"]) == (1, 0, 3)
    assert (r["par_lo"], r["par_hi"], r["ang_lo"], r["ang_hi"]) == (0, 1, 0, 2)
    # keep is formed once as 1.0 - drop, thr is one multiply
    r = one([[3.0, 3.0 * (1.0 - 0.1)]], drop=0.1)
    assert r["n_within"] == 2


# ---- the ground the GPU comparisons stand on --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_live", [("A", 8320), ("B", 3596), ("C", 2370), ("D", 4608), ("F", 12960), ("E", 8780)])
def test_the_oracle_separates_its_two_best_templates(name, n_live):
    live, excluded, _ = ref.oracle_ties(name)
    print(name, int(live.sum()), int(excluded.sum()))
    assert live.sum() == n_live and ((~live).any() or name == "D")          # (a Ricker has no window limits: every cell is live)
    assert excluded.sum() <= 1e-3 * live.sum()


def test_case_e_has_wide_intervals_at_drop_one_half():
    S, A, _, _ = ref.oracle_cubes("E")
    rows = ref.reduce_cube(S, A, 0.5)
    live = rows["status"] != 1
    assert ((rows["par_hi"] - rows["par_lo"])[live] > 1).any() and ((rows["ang_hi"] - rows["ang_lo"])[live] > 1).any()
    # The issue words this as "cells touching both ends of both grids".  What the oracle gives, and what is asserted: each of
    # the four ends is touched by some cell (every bit occurs), and both ends of the AGE grid are touched by one cell
    # (status & 6 == 6).  No cell of the case touches both ends of the ORIENTATION grid at once (no status with 24): that
    # reading of the wording is not asserted, because it does not hold on the oracle.
    assert not (rows["status"][live] & 24 == 24).any()
    st = rows["status"][live]
    assert all((st & b).any() for b in (2, 4, 8, 16)) and (st & 6 == 6).any()
