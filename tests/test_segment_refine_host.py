"""Continuous ages of sl.fit_segments (``refine=``; docs/segments.md, "Continuous ages"), on the CPU: argument validation
before the library is loaded, the layouts of sc_segment_fine_fit and sc_segment_fine_cell and the header's ABI, the park's
formula against the driver's, the new kernels' register and scratch budget, the numpy restatement
(tests/segment_refine_reference.py) in two arithmetics on every input of tests/test_gpu_segment_refine.py - by the rule and
under the cap the GPU test holds the device to -, and what the joint refinement recovers of an age between two grid ages."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import segment_refine_reference as sx
from scarplet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the arguments are validated before the library is loaded -------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    import scarplet_amd.core as core

    def refuse(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(core, "_context", refuse)
    monkeypatch.setattr(_lib, "load", refuse)


def test_refine_validates_before_the_library_is_loaded(no_library):
    import scarplet_amd as sl
    g = sl.DEMGrid.from_array(np.zeros((40, 50)), 2.0)
    ok = dict(data=g, cells=[3, 77], labels=[1, 1], angle=0.1, half_length=20.0)   # h = 10, min_samples = 4
    bad = [
        (dict(refine=-1), "refine < 0"),
        (dict(refine=3), "refine > 2"),
        (dict(refine=True), "a bool"),
        (dict(refine=False), "a bool"),
        (dict(refine=np.True_), "a numpy bool"),
        (dict(refine=1.5), "a float that is not whole"),
        (dict(refine=np.nan), "NaN"),
        (dict(refine=np.inf), "inf"),
        (dict(refine="2"), "a string"),
        (dict(refine=[1]), "a list"),
        (dict(refine=3.0), "a whole float out of range"),
        (dict(refine=1, max_shift=4.0), "with max_shift"),
        (dict(refine=0, max_shift=0), "with max_shift 0"),
        (dict(refine=2, weights=np.ones((40, 50))), "with weights"),
        (dict(refine=1, robust="huber"), "with robust"),
        (dict(refine=1, max_width=4.0), "with max_width"),
        (dict(refine=0, max_width=0), "with max_width 0"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError):
            sl.fit_segments(**dict(ok, **kw))
            pytest.fail(what)
    for kw in (dict(refine=0), dict(refine=1), dict(refine=2, return_curve=True, return_cells=True), dict(refine=np.int64(2)),
               dict(refine=1.0), dict(refine=None), dict()):
        with pytest.raises(AssertionError, match="the library was asked for"):
            sl.fit_segments(**dict(ok, **kw))


def test_matcher_route_validates_refine():
    import scarplet_amd as sl
    from scarplet_amd import traces as tr

    class Held(object):
        whole, ny, nx, de = True, 40, 50, 2.0

        def result_array(self):
            return np.zeros((4, 40, 50))
    labels = np.zeros((40, 50), dtype=np.int32)
    labels[10, 20:24] = 1
    seg = np.zeros(1, dtype=[("label", np.int32), ("strike", np.float64)])
    seg["label"] = 1
    t = tr.Traces(labels > 0, labels, seg)
    for kw in (dict(refine=-1), dict(refine=3), dict(refine=True), dict(refine=0.5), dict(refine=1, max_shift=2.0),
               dict(refine=1, robust="huber"), dict(refine=2, max_width=4.0), dict(refine=2, weights=np.ones((40, 50)))):
        for strike in ("cell", "segment"):
            with pytest.raises(ValueError, match="refine"):
                sl.Matcher.fit_segments(Held(), t, 20.0, strike=strike, **kw)


def test_tables_with_the_fine_fields():
    from scarplet_amd import segments
    assert segments.FINE_FIT_DTYPE.names == segments.FIT_DTYPE.names + sx.FINE_FLOATS + ("status_fine",)
    assert segments.FINE_CELL_DTYPE.names == segments.CELL_DTYPE.names[:-1] + sx.CELL_FLOATS + ("label",)
    assert _lib.SEGMENT_FINE_FLOATS + ("height_fine",) == sx.FINE_FLOATS and _lib.SEGMENT_FINE_CELL_FLOATS == sx.CELL_FLOATS
    # the plain tables are what they were
    assert segments.FIT_DTYPE.names[-1] == "height" and segments.CELL_DTYPE.names[-1] == "label"


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_fine_struct_layouts_match_c(tmp_path):
    pairs = ((_lib.sc_segment_fine_fit, _lib.SEGMENT_FINE_FIT_DTYPE, _lib.sc_segment_fit, "sc_segment_fine_fit"),
             (_lib.sc_segment_fine_cell, _lib.SEGMENT_FINE_CELL_DTYPE, _lib.sc_segment_cell, "sc_segment_fine_cell"))
    body = ""
    for S, dt, T, name in pairs:
        body += '  printf("%%zu\\n", sizeof(%s));\n' % name
        body += "".join('  printf("%%zu\\n", offsetof(%s, %s));\n' % (name, f) for f, _ in S._fields_)
    prog = tmp_path / "fine.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarplet_hip.h"\nint main(void) {\n' + body
                    + '  printf("%d %d %d %d\\n", SC_PROFILE_MAX_REFINE, SC_K_COUNT, SC_ABI_VERSION, SC_SEGMENT_REFINE_COLUMNS);\n'
                    + '  return 0;\n}\n')
    exe = tmp_path / "fine"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = []
    for S, dt, T, name in pairs:
        names = [f for f, _ in S._fields_]
        assert dt.itemsize == ctypes.sizeof(S) and dt.names == tuple(names)
        assert [dt.fields[f][1] for f in names] == [getattr(S, f).offset for f in names]
        want += [ctypes.sizeof(S)] + [getattr(S, f).offset for f in names]
        # the plain struct's fields first, in its layout; the first fine field right behind them
        assert S._fields_[:len(T._fields_)] == T._fields_
        assert all(getattr(S, f).offset == getattr(T, f).offset for f, _ in T._fields_)
        assert getattr(S, names[len(T._fields_)]).offset == ctypes.sizeof(T)
    assert vals == want + [_lib.PROFILE_MAX_REFINE, len(_lib.K_NAMES), 10, _lib.SEGMENT_REFINE_COLUMNS]
    assert [f for f, _ in _lib.sc_segment_fine_fit._fields_][len(_lib.sc_segment_fit._fields_):] == \
        list(_lib.SEGMENT_FINE_FLOATS) + ["status_fine"]
    assert [f for f, _ in _lib.sc_segment_fine_cell._fields_][len(_lib.sc_segment_cell._fields_):] == list(sx.CELL_FLOATS)


REFINE_CALLS = ("sc_fit_segments_refine", "sc_fit_segments_refine_dem")


def test_header_still_says_abi_10_and_declares_the_refine_calls():
    txt = open(os.path.join(ROOT, "include", "scarplet_hip.h")).read()
    assert "#define SC_ABI_VERSION 10\n" in txt and _lib.ABI_VERSION == 10
    assert re.search(r"#define\s+SC_K_COUNT\s+11\b", txt) and len(_lib.K_NAMES) == 11
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in REFINE_CALLS:
        assert re.search(r"\bint %s\s*\(" % n, code), n


def test_library_exports_the_refine_calls():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in REFINE_CALLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    # the plain call's arguments with R after w; the _dem form takes (z, ny, nx) ahead of the same arguments
    a, b = _lib.SIGNATURES["sc_fit_segments_refine"][1], _lib.SIGNATURES["sc_fit_segments_refine_dem"][1]
    p = _lib.SIGNATURES["sc_fit_segments"][1]
    assert a[:12] + a[13:] == p and a[12] is ctypes.c_int and b[:1] + b[4:] == a
    assert _lib.load().sc_abi_version() == 10
    assert hasattr(_lib.Context, "fit_segments_refine")


def test_build_id_covers_the_new_source():
    mk = open(os.path.join(ROOT, "scarplet_amd", "csrc", "Makefile")).read()
    src = re.search(r"^SRC\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "sc_segment_refine.hip" in src and re.search(r"^ID_SRC\s*=\s*\$\(SRC\)", mk, flags=re.M)
    # one definition of the candidates' column for both files
    fit_h = open(os.path.join(ROOT, "scarplet_amd", "csrc", "sc_fit.h")).read()
    assert "struct rf_col" in fit_h and "rf_x(" in fit_h and "#define RF_SAT" in fit_h
    for f in ("sc_refine.hip", "sc_segment_refine.hip"):
        txt = open(os.path.join(ROOT, "scarplet_amd", "csrc", f)).read()
        assert "struct rf_col" not in txt and "#define RF_SAT" not in txt and "rf_col{" in txt, f


# ---- the park -----------------------------------------------------------------------------------------------------------------
def test_the_park_cap_is_the_one_of_the_python_side(tmp_path, monkeypatch):
    """sc_fit_park_cap (tests/fit_chunk_check.cpp, a program of its own under AddressSanitizer and UBSan) in the shape the
    driver describes this call's park - planes = 4, C = A + Cc - against _lib.segment_refine_cap and segments.check_refine: a
    segment of `cap` cells passes and one of cap + 1 is refused with both numbers in the message."""
    from scarplet_amd import segments
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ builds this test's program: it is not on PATH"
    exe = str(tmp_path / "fit_chunk_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "fit_chunk_check.cpp"), "-o", exe], check=True)
    full = _lib.SEGMENT_MAX_PARK
    grid = [(A, h, R, full) for A in (1, 2, 35, 64) for h in (5, 100, 1024) for R in (0, 1, 2)]
    grid += [(2, 10, 1, 40 * 8 * (21 + 4 * 130)), (2, 10, 0, 40 * 8 * (21 + 4 * 2)), (5, 7, 2, 100000)]
    Cc = lambda R: _lib.SEGMENT_REFINE_COLUMNS if R > 0 else 0
    text = "".join("%d %d %d %d %d\n" % (park, 2 * h + 1, 4, A + Cc(R), 0) for A, h, R, park in grid)
    r = subprocess.run([exe, "cap"], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    caps = [int(v) for v in r.stdout.split()]
    assert len(caps) == len(grid)
    for (A, h, R, park), cap in zip(grid, caps):
        assert cap == park // (8 * ((2 * h + 1) + 4 * (A + Cc(R))))            # the issue's formula, written out
        monkeypatch.setattr(_lib, "SEGMENT_MAX_PARK", park)
        assert _lib.segment_refine_cap(h, A, R) == cap

        def args(n):                                     # (what check_refine reads of check_args' record)
            blank = segments.Args(*[None] * len(segments.Args._fields))
            return blank._replace(seg_start=np.array([0, 3, 3 + n]), ages=np.ones(A), h=h)
        assert segments.check_refine(args(cap), R) == R
        with pytest.raises(ValueError, match="a segment of %d cells: more than %d at" % (cap + 1, cap)):
            segments.check_refine(args(cap + 1), R)
        assert segments.check_refine(args(cap + 1), None) is None
    assert _lib.SEGMENT_REFINE_COLUMNS == 128
    src = open(os.path.join(ROOT, "scarplet_amd", "csrc", "sc_segment_refine.hip")).read()
    assert re.search(r"sg_park_plain\(A \+ \(R > 0 \? SX_COLUMNS : 0\), h, false\)", src)


# ---- the kernels' budget -------------------------------------------------------------------------------------------------------
def test_the_new_kernels_have_no_scratch_and_three_waves_per_simd():
    from test_isa_budget import kernel_table
    t = kernel_table("sc_segment_refine.hip")
    for k in ("k_sx_begin", "k_sx_column", "k_sx_resid", "k_sx_pick", "k_sx_finish"):
        assert k in t, sorted(t)
        assert t[k]["scratch"] == 0, (k, t[k])
        assert t[k]["vgpr"] + t[k]["agpr"] <= 168, (k, t[k])
    print({k: t[k] for k in sorted(t)})


# ---- the restatement --------------------------------------------------------------------------------------------------------
def test_the_case_list():
    cases = sx.gpu_cases()
    assert [c["name"] for c in cases] == sx.NAMES
    by = {c["name"]: c for c in cases}
    c = by["synthetic"]
    assert (c["h"], c["w"]) == (100, 2) and len(c["cells"]) == 120 and len(np.unique(c["labels"])) == 8
    c = by["sizes 1 2 64 65 130"]
    assert (c["h"], c["w"]) == (5, 1) and list(c["ages"]) == [1.0, 3.0]
    assert sorted(np.unique(c["labels"], return_counts=True)[1]) == [1, 2, 64, 65, 130]
    assert len(by["one age"]["ages"]) == 1 and len(by["64 ages"]["ages"]) == 64 and len(by["no cell"]["cells"]) == 0
    assert 8 * (2 * by["64 ages"]["h"] + 1) * 64 > 65536                   # the table in global memory
    assert np.all(by["labels <= 0 only"]["labels"] <= 0) and by["min_profiles 25"]["min_profiles"] == 25
    assert np.isnan(by["NaN cells and borders"]["z"]).any()
    assert by["repeated cells"]["delta"] == 0.0
    c = by["120 segments of 3"]
    assert c["h"] == 15 and 1 < len(c["ages"]) <= 35 and np.all(np.unique(c["labels"], return_counts=True)[1] == 3)
    assert len(np.unique(c["labels"])) == 120
    assert by["h1024"]["h"] == 1024 and len(by["h1024"]["cells"]) == 4 and len(np.unique(by["h1024"]["labels"])) == 1


@pytest.mark.parametrize("name", sx.NAMES)
def test_the_restatement_in_two_arithmetics(name):
    """Float64 lstsq on the full design matrix per candidate against longdouble per-profile orthogonalisation per candidate,
    by the rule of the GPU test - and the condition on the inputs that the rule rests on: the two arithmetics part in NO
    segment, and the segments with any margin below 1e-8 (where two implementations that are each within RTOL could part) stay
    within the tie cap: none in a case under 100 segments."""
    case = sx.gpu_cases()[sx.NAMES.index(name)]
    for R in sx.LEVELS:
        ref = sx.reference(name, R)
        other = sx.restate(case, R, fit=sx.fit_age_longdouble)
        st = sx.compare(ref, other, case, R)
        close = sx.close_margins(ref)
        print("%s, R = %d: %s, %d segments with a margin below %g" % (name, R, st, close, sx.MARGIN_MIN))
        assert st["ties"] == 0
        assert close <= sx.TIE_SHARE * len(ref), (name, R, close, [r["margin"] for r in ref if r["status"] != 1])
        assert st["fitted"] > 0 or name in ("no cell", "labels <= 0 only")
        if name in ("min_profiles 25", "unusable segment"):
            assert 0 < st["fitted"] < st["segments"]
        if name == "best age below the grid":
            assert all(r["kt_index"] == 0 and r["status_fine"] & 2 for r in ref)
        if name == "best age above the grid":
            assert all(r["kt_index"] == len(case["ages"]) - 1 and r["status_fine"] & 4 for r in ref)
        if name == "one age":
            assert all(r["kt_fine"] == case["ages"][0] == r["kt_lo_fine"] == r["kt_hi_fine"] and r["status_fine"] == 6 for r in ref)


def test_no_level_is_the_grid():
    case = sx.gpu_cases()[sx.NAMES.index("one age")]
    for r in sx.restate(case, 0):
        assert (r["kt_fine"], r["kt_lo_fine"], r["kt_hi_fine"]) == (r["kt"], r["kt_lo"], r["kt_hi"])
        assert (r["a_fine"], r["sse_fine"], r["rmse_fine"]) == (r["a"], r["sse"], r["rmse"])
        assert r["status_fine"] == r["status"] and r["height_fine"] == 2.0 * r["a"]


def test_a_segment_of_one_profile_is_the_cell_of_refine_reference():
    """The joint restatement on one profile picks what tests/refine_reference.py picks for the cell."""
    import refine_reference as rf
    c = rf.gpu_cases()[0]
    one = dict(c, cells=c["cells"][:3], angle=c["angle"][:3], labels=np.arange(1, 4), min_profiles=1)
    for r, q in zip(sx.restate(one, 2), rf.restate(dict(c, cells=c["cells"][:3], angle=c["angle"][:3]), 2)):
        assert (r["kt_fine"], r["kt_lo_fine"], r["kt_hi_fine"], r["status_fine"]) == \
            (q["kt_fine"], q["kt_lo_fine"], q["kt_hi_fine"], q["status_fine"])
        assert abs(r["sse_fine"] - q["sse_fine"]) <= sx.RTOL * q["sse_fine"]


# ---- what it recovers (docs/segments.md, "Continuous ages") -----------------------------------------------------------------
@pytest.mark.parametrize("sigma", sx.SIGMAS)
def test_recovery_of_an_age_between_two_grid_ages(sigma):
    """synthetic_scarp(600, theta=0.2, kt0=10**1.05), the 100 cells on the line as ONE segment, h = 100, w = 2, R = 2: the
    restatement's |kt_fine / kt0 - 1| is below a third of the grid's |kt / kt0 - 1|.  Measured (also in docs/segments.md): the
    grid is off by 12.2 %, 12.2 % and 10.9 % at noise 0, 0.05 and 0.5, kt_fine by 0.77 %, 0.46 % and 2.2 % - ratios of 0.064,
    0.038 and 0.205; the smallest margin of the minimum's two levels is 1.5e-6, 1.8e-7 and 3.9e-9."""
    case = sx.recovery_case(sigma)
    row = sx.restate(case, 2)[0]
    grid_off, fine_off = sx.recovery_figures(row)
    print("sigma %g: grid off by %.4g, fine off by %.4g, ratio %.3g, margins %s" % (sigma, grid_off, fine_off, fine_off / grid_off,
                                                                                     row["margin"]))
    assert row["status"] != 1 and row["n_profiles"] == 100
    assert row["sse_fine"] <= row["sse"] and row["kt_lo_fine"] <= row["kt_fine"] <= row["kt_hi_fine"]
    assert fine_off < grid_off / 3.0
