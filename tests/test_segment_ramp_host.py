"""The initial slope of sl.fit_segments (docs/segments.md, "The initial slope"), on the CPU: argument validation of
``max_width``, ``initial_slope`` and ``return_width`` before the library is loaded, the layout of sc_segment_ramp_fit, the
header's ABI, the Makefile, the kernels' scratch budget, the two numpy restatements (tests/segment_ramp_reference.py)
against each other on every input of tests/test_gpu_segment_ramp.py, and what the shared width recovers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ramp_reference as rr
import segment_ramp_reference as sx
import segment_reference as sr
from scarplet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the arguments are validated before the library is loaded -------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    import scarplet_amd.core as core

    def refuse(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(core, "_context", refuse)
    monkeypatch.setattr(_lib, "load", refuse)


def test_max_width_validates_before_the_library_is_loaded(no_library):
    import scarplet_amd as sl
    g = sl.DEMGrid.from_array(np.zeros((40, 50)), 2.0)
    ok = dict(data=g, cells=[3, 77, 78], labels=[1, 2, 2], angle=0.1, half_length=20.0)      # h = 10, min_samples = 4
    bad = [
        (dict(max_width=-1.0), "max_width < 0"),
        (dict(max_width=np.nan), "max_width NaN"),
        (dict(max_width=np.inf), "max_width inf"),
        (dict(max_width="wide"), "max_width not a number"),
        (dict(max_width=True), "max_width a bool"),
        (dict(max_width=14.0), "7 cells, more than h - min_samples = 6"),
        (dict(max_width=12.0, min_samples=5), "6 cells, more than h - min_samples = 5"),
        (dict(max_width=2.0 * 65, half_length=400.0), "65 cells, more than 64"),
        (dict(initial_slope=0.6), "initial_slope without max_width"),
        (dict(return_width=True), "return_width without max_width"),
        (dict(max_width=None, return_width=True), "return_width with max_width None"),
        (dict(max_width=8.0, initial_slope=0.0), "a slope of 0"),
        (dict(max_width=8.0, initial_slope=-0.6), "a negative slope: it is a magnitude"),
        (dict(max_width=8.0, initial_slope=np.nan), "a NaN slope"),
        (dict(max_width=8.0, initial_slope=np.inf), "an infinite slope"),
        (dict(max_width=8.0, initial_slope="steep"), "a slope that is no number"),
        (dict(max_width=8.0, initial_slope=True), "a slope that is a bool"),
        (dict(max_width=1.9, initial_slope=0.6), "a slope with M = 0"),
        (dict(max_width=0, initial_slope=0.6), "a slope with max_width 0"),
        (dict(max_width=8.0, max_shift=4.0), "with max_shift"),
        (dict(max_width=8.0, max_shift=0), "with max_shift 0"),
        (dict(max_width=0, max_shift=2.0, return_shift=True), "max_width 0 with max_shift"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError):
            sl.fit_segments(**dict(ok, **kw))
            pytest.fail(what)
    # what is valid gets as far as the device: the whole range, the largest width the call takes, zero, both modes
    for kw in (dict(max_width=13.9), dict(max_width=2.0 * 64, half_length=400.0), dict(max_width=0),
               dict(max_width=0.0, return_width=True), dict(max_width=2.0, initial_slope=0.6),
               dict(max_width=12.0, initial_slope=1e-3, return_width=True, return_curve=True, return_cells=True), dict()):
        with pytest.raises(AssertionError, match="the library was asked for"):
            sl.fit_segments(**dict(ok, **kw))


def test_the_park_cap_counts_the_pairs(no_library, monkeypatch):
    """8 ((2h + 1) + 4 A (M + 1)) bytes per cell against SC_SEGMENT_MAX_PARK, a segment at a time."""
    import scarplet_amd as sl
    from scarplet_amd import segments
    h, A, M = 100, 35, 8
    per = 8 * ((2 * h + 1) + 4 * A * (M + 1))
    assert per == 11688 and _lib.SEGMENT_MAX_PARK // per // 1000 == 367       # 11.7 KB per cell, 367 thousand cells
    # a park of 40 cells at h = 10, two ages, M = 6: segments of 40 pass, 41 do not - and pass without the width
    per = 8 * (21 + 4 * 2 * 7)
    monkeypatch.setattr(_lib, "SEGMENT_MAX_PARK", 40 * per)
    g = sl.DEMGrid.from_array(np.zeros((40, 50)), 2.0)
    kw = dict(data=g, angle=0.1, half_length=20.0, ages=[1.0, 2.0])
    with pytest.raises(AssertionError, match="the library was asked for"):
        sl.fit_segments(cells=np.arange(80), labels=np.repeat([1, 2], 40), max_width=12.0, **kw)
    with pytest.raises(ValueError, match="a segment of 41 cells: more than 40"):
        sl.fit_segments(cells=np.arange(81), labels=np.repeat([1, 2], [40, 41]), max_width=12.0, **kw)
    with pytest.raises(AssertionError, match="the library was asked for"):
        sl.fit_segments(cells=np.arange(81), labels=np.repeat([1, 2], [40, 41]), **kw)
    args = segments.check_args((40, 50), 2.0, np.arange(81), np.repeat([1, 2], [40, 41]), 0.1, 20.0, 0, [1.0, 2.0], 1.0, 4, 1)
    segments.check_park(args, 5)
    with pytest.raises(ValueError):
        segments.check_park(args, 6)


def test_matcher_route_validates_max_width():
    import scarplet_amd as sl
    from scarplet_amd import traces

    class Held(object):
        whole, ny, nx, de = True, 40, 50, 2.0

        def result_array(self):
            return [None, None, np.full((40, 50), 0.1)]
    lab = np.zeros((40, 50), dtype=np.int32)
    lab[20, 10:30] = 1
    tr = traces.Traces(lab > 0, lab, None)
    for kw in (dict(max_width=-1.0), dict(max_width=14.0), dict(return_width=True), dict(initial_slope=0.6),
               dict(max_width=8.0, initial_slope=-1.0), dict(max_width=8.0, max_shift=2.0)):
        with pytest.raises(ValueError, match="width|slope"):
            sl.Matcher.fit_segments(Held(), tr, 20.0, **kw)


def test_table_with_the_width():
    from scarplet_amd import segments
    names = segments.FIT_DTYPE.names
    assert segments.RAMP_FIT_DTYPE.names == names[:-1] + ("width_index", "width", "initial_slope", "height")
    assert segments.RAMP_FIT_DTYPE.names[:-1] == _lib.SEGMENT_RAMP_FIT_DTYPE.names


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_segment_ramp_struct_layout_matches_c(tmp_path):
    S, dt = _lib.sc_segment_ramp_fit, _lib.SEGMENT_RAMP_FIT_DTYPE
    names = [f for f, _ in S._fields_]
    body = '  printf("%zu\\n", sizeof(sc_segment_ramp_fit));\n'
    body += "".join('  printf("%%zu\\n", offsetof(sc_segment_ramp_fit, %s));\n' % f for f in names)
    prog = tmp_path / "segramp.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarplet_hip.h"\nint main(void) {\n' + body
                    + '  printf("%zu %lld %d %d\\n", sizeof(sc_segment_cell), SC_SEGMENT_MAX_PARK >> 32, SC_K_COUNT, SC_ABI_VERSION);\n'
                    + '  return 0;\n}\n')
    exe = tmp_path / "segramp"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [ctypes.sizeof(S)] + [getattr(S, f).offset for f in names]
    assert dt.itemsize == ctypes.sizeof(S) and dt.names == tuple(names)
    assert [dt.fields[f][1] for f in names] == [getattr(S, f).offset for f in names]
    # no new timing slot, the ABI as it was, the cell table's struct the plain call's
    assert vals == want + [ctypes.sizeof(_lib.sc_segment_cell), 1, len(_lib.K_NAMES), 10]
    # the shared fields sit where sc_segment_fit has them
    T = _lib.sc_segment_fit
    assert S._fields_[:len(T._fields_)] == T._fields_
    assert all(getattr(S, f).offset == getattr(T, f).offset for f, _ in T._fields_)
    assert names[-3:] == ["width_index", "width", "initial_slope"]


CALLS = ("sc_fit_segments_ramp", "sc_fit_segments_ramp_dem")


def test_header_still_says_abi_10_and_declares_the_calls():
    txt = open(os.path.join(ROOT, "include", "scarplet_hip.h")).read()
    assert "#define SC_ABI_VERSION 10\n" in txt and _lib.ABI_VERSION == 10
    assert re.search(r"#define\s+SC_K_COUNT\s+11\b", txt) and len(_lib.K_NAMES) == 11
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in CALLS:
        assert re.search(r"\bint %s\s*\(" % n, code), n


def test_library_exports_the_calls():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in CALLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    # the _dem form takes (z, ny, nx) ahead of the same arguments; the call is sc_fit_segments' with M, mode, slope and a plane
    a, b = _lib.SIGNATURES["sc_fit_segments_ramp"][1], _lib.SIGNATURES["sc_fit_segments_ramp_dem"][1]
    assert len(a) == len(_lib.SIGNATURES["sc_fit_segments"][1]) + 4 and b[:1] + b[4:] == a
    assert _lib.load().sc_abi_version() == 10


def test_the_makefile_lists_the_source():
    mk = open(os.path.join(ROOT, "scarplet_amd", "csrc", "Makefile")).read()
    src = re.search(r"^SRC\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "sc_segment_ramp.hip" in src and os.path.exists(os.path.join(ROOT, "scarplet_amd", "csrc", "sc_segment_ramp.hip"))


def test_segment_ramp_kernels_have_no_scratch():
    from test_isa_budget import kernel_table
    t = kernel_table("sc_segment_ramp.hip")
    # (the segmented sum over the A (M + 1) columns is sc_segment.hip's k_sg_sum1<2> / k_sg_sum2<2>)
    t.update({k: v for k, v in kernel_table("sc_segment.hip").items() if k.startswith("k_sg_sum")})
    for k in ("k_sr_partial<true>", "k_sr_partial<false>", "k_sr_resid<true>", "k_sr_resid<false>", "k_sr_choose",
              "k_sg_sum1<2>", "k_sg_sum2<2>"):
        assert k in t, sorted(t)
        assert t[k]["scratch"] == 0, (k, t[k])
        assert t[k]["vgpr"] + t[k]["agpr"] <= 128, (k, t[k])               # four waves per SIMD


# ---- the restatements ---------------------------------------------------------------------------------------------------------
def test_the_case_list():
    cases = sx.gpu_cases()
    assert [c["name"] for c in cases] == sx.NAMES
    for c in cases:
        assert 0 <= c["M"] <= min(_lib.PROFILE_MAX_WIDTH, c["h"] - c["min_samples"]) and len(c["cells"]) <= 500
        assert max(c["z"].shape) <= 600 and c["slope"] > 0
    by = {c["name"]: c for c in cases}
    assert {(by[n]["h"], by[n]["w"], by[n]["M"]) for n in sx.NAMES[:2]} == {(100, 0, 8), (30, 5, 4)}
    assert all(len(np.unique(by[n]["labels"])) == 8 for n in sx.NAMES[:2])
    c = by["h100 w0 M8"]
    assert len(c["ages"]) * (c["M"] + 1) == 315                                # five rounds, the last one partial
    assert 8 * (2 * (c["h"] + c["M"]) + 1) * len(c["ages"]) <= 65536            # the table in LDS
    c = by["64 ages M1"]
    assert len(c["ages"]) == 64 and 8 * (2 * (c["h"] + c["M"]) + 1) * 64 > 65536  # ... and in global memory
    c = by["sizes 1 2 64 65 130"]
    rows = sx.restate(c, sx.FREE, longdouble=True)
    assert sorted(r["n_profiles"] for r in rows) == [1, 2, 64, 65, 130]        # usable, not cells alone
    assert (c["h"], c["M"], len(c["ages"])) == (12, 2, 2)
    c = by["M = h - min_samples"]
    assert c["M"] == c["h"] - c["min_samples"]
    assert len(by["one age M8"]["ages"]) == 1 and by["de 2"]["de"] == 2.0
    assert len(by["no cell"]["cells"]) == 0 and by["labels <= 0 only"]["labels"].max() <= 0
    rows = sx.restate(by["unusable segment"], sx.FREE, longdouble=True)
    assert [r["n_profiles"] for r in rows] == [0, 2] and [r["status"] & 1 for r in rows] == [1, 0]
    rows = sx.restate(by["min_profiles 5"], sx.FREE, longdouble=True)
    assert sorted(r["status"] & 1 for r in rows) == [0, 0, 0, 1, 1, 1]


def test_the_dof_case_has_the_segment_it_is_about():
    case = {c["name"]: c for c in sx.gpu_cases()}["dof < 1 with the width free"]
    free, given = sx.restate(case, sx.FREE), sx.restate(case, sx.SLOPE)
    assert (free[0]["n_profiles"], free[0]["n"], free[0]["dof"], free[0]["status"]) == (1, 4, 0, 1)
    assert given[0]["dof"] == 1 and given[0]["status"] != 1 and given[0]["width_index"] == 1
    assert free[1]["n_profiles"] == 3 and free[1]["dof"] == 21 - 6 - 2 and free[1]["status"] != 1


@pytest.mark.parametrize("name", sx.NAMES)
def test_the_two_restatements_agree(name):
    """Float64 lstsq on the equilibrated full design matrix against per-profile longdouble Gram-Schmidt on a longdouble
    table, on every input of the GPU tests: RTOL / 100 in every pooled sse_im, every profile's share of it and every
    coefficient (relative to the largest range of a profile), every compared pair under the condition cap, and no m_i, no
    index and no status decided differently in either mode.  The age grids of the cases are cut to where this holds
    (segment_ramp_reference.NA)."""
    case = {c["name"]: c for c in sx.gpu_cases()}[name]
    a, b = sx.case_pairs(case), sx.case_pairs(case, longdouble=True)
    worst = {"sse": 0.0, "coef": 0.0, "cond": 0.0, "segments": 0}
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x["n"] == y["n"] and x["n_profiles"] == y["n_profiles"] and np.array_equal(x["used"], y["used"])
        if not x["n_profiles"]:
            continue
        worst["segments"] += 1
        assert x["cond"] <= sx.COND_MAX, (x["label"], x["cond"])
        gy = y["grid"].astype(np.float64)
        f64 = lambda v: v.astype(np.float64)
        hd = case["h"] * case["de"]
        worst["sse"] = max(worst["sse"], float(np.max(np.abs(x["grid"] - gy) / gy)),
                           float(np.max(np.abs(x["per"] - f64(y["per"])) / gy[..., None])))
        worst["coef"] = max(worst["coef"], float(max(np.max(np.abs(x["a_all"] - f64(y["a_all"]))), np.max(np.abs(x["c0_all"] - f64(y["c0_all"]))),
                                                     np.max(np.abs(x["b_all"] - f64(y["b_all"]))) * hd)) / x["ptp"])
        worst["cond"] = max(worst["cond"], x["cond"])
    print("%s: %s" % (name, worst))
    assert worst["sse"] <= sx.RTOL / 100 and worst["coef"] <= sx.RTOL / 100, worst
    for mode in (sx.FREE, sx.SLOPE):
        for x, y in zip(sx.restate(case, mode), sx.restate(case, mode, longdouble=True)):
            for f in ("n", "dof", "kt_index", "lo_index", "hi_index", "status", "width_index"):
                assert x[f] == y[f], (name, mode, x["label"], f, x[f], y[f])
            assert np.array_equal(x["widths"], y["widths"]), (name, mode, x["label"])


def test_width_zero_is_the_plain_restatement():
    case = {c["name"]: c for c in sx.gpu_cases()}["h30 w5 M4"]
    plain = sr.fit_segments(case["z"], 1.0, case["cells"], case["labels"], case["angle"], 30, 5, case["ages"], 1.0, 15)
    zero = sx.fit_segments(case["z"], 1.0, case["cells"], case["labels"], case["angle"], 30, 5, 0, case["ages"], min_samples=15)
    assert len(zero) == len(plain) == 8
    for x, y in zip(zero, plain):
        assert x["width_index"] == 0 and x["width"] == 0.0 and np.isinf(x["initial_slope"])
        for f in ("label", "n_cells", "n_profiles", "n", "dof", "kt_index", "lo_index", "hi_index", "status"):
            assert x[f] == y[f], f
        assert abs(x["sse"] - y["sse"]) <= 1e-11 * y["sse"] and abs(x["a"] - y["a"]) <= 1e-11


def test_one_profile_is_the_single_profile_restatement():
    """A segment of one usable profile is ramp_reference's cell: the same design matrix."""
    case = {c["name"]: c for c in sx.gpu_cases()}["h30 w5 M4"]
    k = 3
    for mode in (sx.FREE, sx.SLOPE):
        one = sx.fit_segments(case["z"], 1.0, case["cells"][k:k + 1], [7], case["angle"][k:k + 1], 30, 5, 4, case["ages"], mode,
                              case["slope"], min_samples=15)[0]
        cell = rr.fit_profiles(case["z"], 1.0, case["cells"][k:k + 1], case["angle"][k:k + 1], 30, 5, 4, case["ages"], mode,
                               case["slope"], min_samples=15)[0]
        for f in ("n", "dof", "kt_index", "lo_index", "hi_index", "status", "width_index"):
            assert one[f] == cell[f], (mode, f)
        assert np.array_equal(one["widths"], cell["widths"])
        assert abs(one["sse"] - cell["sse"]) <= 1e-11 * cell["sse"] and abs(one["initial_slope"] - cell["initial_slope"]) <= 1e-11


# ---- what it does: the recovery surface of docs/segments.md --------------------------------------------------------------------
def test_the_shared_width_finds_the_age_the_plain_joint_fit_misses():
    """ramp_reference.recovery_case(): 600 x 600, theta = 0.2, a ramp of half-width 6 cells diffused for ages[10], noise
    0.02, its 100 cells one segment, h = 100, w = 2, M = 8.  The plain joint fit: index 12.  The width free and the slope
    given: index 10, width_index 6, interval [10, 10].  Asserted on the lstsq restatement; the longdouble twin gives the same
    rows."""
    R = rr.REC
    z, cells, theta, ages = rr.recovery_case()
    assert len(cells) == 100
    plain = sr.fit_segments(z, 1.0, cells, np.ones(100, dtype=np.int64), theta, R["h"], R["w"], ages)[0]
    assert plain["kt_index"] == 12 and plain["n_profiles"] == 100
    pairs = sx.pairs_of_segments(z, 1.0, cells, np.ones(100, dtype=np.int64), theta, R["h"], R["w"], R["M"], ages)
    assert pairs[0]["cond"] <= sx.COND_MAX
    for mode in (sx.FREE, sx.SLOPE):
        row = sx.fit_segments(z, 1.0, cells, None, theta, R["h"], R["w"], R["M"], ages, mode, R["slope"], pairs=pairs)[0]
        twin = sx.recovery_rows(R["noise"], mode)[0]
        print("mode %d: index %d, m = %d, [%d, %d], a = %.5f, slope %.5f" % (mode, row["kt_index"], row["width_index"],
                                                                          row["lo_index"], row["hi_index"], row["a"], row["initial_slope"]))
        for r in (row, twin):
            assert (r["kt_index"], r["width_index"], r["lo_index"], r["hi_index"]) == (R["index"], R["L"], R["index"], R["index"])
            assert r["status"] == 0 and r["dof"] == r["n"] - 200 - 1 - (1 if mode == sx.FREE else 0)
        assert abs(row["a"] - 1.0) <= 0.01 and abs(row["initial_slope"] - (-0.01 + 1.0 / 6.0)) <= 2e-3


def test_segments_of_25_cells_recover_age_and_width_at_noise_005():
    R = rr.REC
    z, cells, theta, ages = rr.recovery_case(0.05)
    rows = sx.fit_segments(z, 1.0, cells, np.arange(100) // 25 + 1, theta, R["h"], R["w"], R["M"], ages)
    assert len(rows) == 4 and all(r["n_profiles"] == 25 for r in rows)
    assert [(r["kt_index"], r["width_index"]) for r in rows] == [(R["index"], R["L"])] * 4
    assert [(r["kt_index"], r["width_index"]) for r in sx.recovery_rows(0.05, sx.FREE, size=25)] == [(R["index"], R["L"])] * 4
    # the whole line at noise 0.05, both modes (the longdouble twin)
    for mode in (sx.FREE, sx.SLOPE):
        r = sx.recovery_rows(0.05, mode)[0]
        assert (r["kt_index"], r["width_index"], r["lo_index"], r["hi_index"]) == (R["index"], R["L"], R["index"], R["index"])
