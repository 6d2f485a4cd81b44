"""Continuous ages of sl.fit_profiles (``refine=``; docs/profiles.md, "Continuous ages"), on the CPU: argument validation
before the library is loaded, the layout of sc_profile_fine_fit and the header's ABI, the kernel's scratch budget, the numpy
restatement (tests/refine_reference.py) in two arithmetics on every input of tests/test_gpu_refine.py - by the rule and
under the cap the GPU test holds the device to -, and what the refinement recovers of an age between two grid ages."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import profile_reference as pr
import refine_reference as rf
from scarplet_amd import _lib, _plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    ok = dict(data=g, cells=[3, 77], angle=0.1, half_length=20.0)                  # h = 10, min_samples = 4
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
            sl.fit_profiles(**dict(ok, **kw))
            pytest.fail(what)
    for kw in (dict(refine=0), dict(refine=1), dict(refine=2, return_curve=True), dict(refine=np.int64(2)), dict(refine=1.0),
               dict(refine=None), dict()):
        with pytest.raises(AssertionError, match="the library was asked for"):
            sl.fit_profiles(**dict(ok, **kw))


def test_check_refine():
    from scarplet_amd import profiles
    assert profiles.check_refine(None) is None
    assert [profiles.check_refine(v) for v in (0, 1, 2, 2.0, np.int32(1))] == [0, 1, 2, 2, 1]
    assert _lib.PROFILE_MAX_REFINE == 2
    # None leaves the other options alone
    assert profiles.check_refine(None, max_shift=2.0, weights=1, robust="huber", max_width=3.0) is None


def test_matcher_route_validates_refine():
    import scarplet_amd as sl

    class Held(object):
        whole, ny, nx, de = True, 40, 50, 2.0
    for kw in (dict(refine=-1), dict(refine=3), dict(refine=True), dict(refine=0.5), dict(refine=1, max_shift=2.0),
               dict(refine=1, robust="huber"), dict(refine=2, max_width=4.0), dict(refine=2, weights=np.ones((40, 50)))):
        with pytest.raises(ValueError, match="refine"):
            sl.Matcher.fit_profiles(Held(), [3, 77], 20.0, angle=0.1, **kw)


def test_table_with_the_fine_fields():
    from scarplet_amd import profiles
    assert profiles.FINE_FIT_DTYPE.names == profiles.FIT_DTYPE.names + rf.FINE_FLOATS + ("status_fine",)
    assert _lib.FINE_FLOATS == rf.FINE_FLOATS
    rows = np.zeros(2, dtype=_lib.PROFILE_FINE_DTYPE)
    rows["cell"], rows["a"], rows["kt_fine"], rows["status_fine"] = [7, 53], [0.5, -1.0], [11.0, 12.0], [2, 4]
    t = profiles._table(rows, 50, label=[3, 3])
    assert t.dtype.names == profiles.FINE_FIT_DTYPE.names + ("label",)
    assert list(t["row"]) == [0, 1] and list(t["col"]) == [7, 3] and list(t["height"]) == [1.0, -2.0]
    assert list(t["kt_fine"]) == [11.0, 12.0] and list(t["status_fine"]) == [2, 4]
    # the plain table is what it was
    plain = profiles._table(np.zeros(1, dtype=_lib.PROFILE_DTYPE), 50)
    assert plain.dtype == profiles.FIT_DTYPE


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_fine_struct_layout_matches_c(tmp_path):
    S, dt = _lib.sc_profile_fine_fit, _lib.PROFILE_FINE_DTYPE
    names = [f for f, _ in S._fields_]
    body = '  printf("%zu\\n", sizeof(sc_profile_fine_fit));\n'
    body += "".join('  printf("%%zu\\n", offsetof(sc_profile_fine_fit, %s));\n' % f for f in names)
    prog = tmp_path / "fine.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarplet_hip.h"\nint main(void) {\n' + body
                    + '  printf("%d %d %d\\n", SC_PROFILE_MAX_REFINE, SC_K_COUNT, SC_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "fine"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert dt.itemsize == ctypes.sizeof(S) and dt.names == tuple(names)
    assert [dt.fields[f][1] for f in names] == [getattr(S, f).offset for f in names]
    assert vals == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in names] + [_lib.PROFILE_MAX_REFINE, len(_lib.K_NAMES), 10]
    # the fields of sc_profile_fit first, in its layout; the first fine field right behind them
    T = _lib.sc_profile_fit
    assert S._fields_[:len(T._fields_)] == T._fields_
    assert all(getattr(S, f).offset == getattr(T, f).offset for f, _ in T._fields_)
    assert names[len(T._fields_)] == "kt_fine" and S.kt_fine.offset == ctypes.sizeof(T)
    assert names[len(T._fields_):] == list(rf.FINE_FLOATS) + ["status_fine"]


REFINE_CALLS = ("sc_fit_profiles_refine", "sc_fit_profiles_refine_dem")


def test_header_still_says_abi_10_and_declares_the_refine_calls():
    txt = open(os.path.join(ROOT, "include", "scarplet_hip.h")).read()
    assert "#define SC_ABI_VERSION 10\n" in txt and _lib.ABI_VERSION == 10
    assert re.search(r"#define\s+SC_K_COUNT\s+11\b", txt) and len(_lib.K_NAMES) == 11
    assert re.search(r"#define\s+SC_PROFILE_MAX_REFINE\s+2\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in REFINE_CALLS:
        assert re.search(r"\bint %s\s*\(" % n, code), n


def test_library_exports_the_refine_calls():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in REFINE_CALLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    # the plain call's arguments with R after w; the _dem form takes (z, ny, nx) ahead of the same arguments
    a, b = _lib.SIGNATURES["sc_fit_profiles_refine"][1], _lib.SIGNATURES["sc_fit_profiles_refine_dem"][1]
    p = _lib.SIGNATURES["sc_fit_profiles"][1]
    assert a[:9] + a[10:] == p and a[9] is ctypes.c_int and b[:1] + b[4:] == a
    assert _lib.load().sc_abi_version() == 10


def test_build_id_covers_the_new_source():
    mk = open(os.path.join(ROOT, "scarplet_amd", "csrc", "Makefile")).read()
    src = re.search(r"^SRC\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "sc_refine.hip" in src and re.search(r"^ID_SRC\s*=\s*\$\(SRC\)", mk, flags=re.M)


def test_refine_kernel_has_no_scratch():
    from test_isa_budget import kernel_table
    t = kernel_table("sc_refine.hip")
    for k in ("k_pf_refine<true>", "k_pf_refine<false>"):
        assert k in t, sorted(t)
        assert t[k]["scratch"] == 0, (k, t[k])
        assert t[k]["vgpr"] + t[k]["agpr"] <= 256, (k, t[k])               # two waves per SIMD: what the LDS of the default shape allows


# ---- the restatement --------------------------------------------------------------------------------------------------------
def test_the_candidates_are_the_definition():
    x = rf.candidates(3.0, 7.5)
    assert x[0] == 3.0 and x[63] == 7.5 and np.all(np.diff(x) > 0)
    assert x[31] == 3.0 + (7.5 - 3.0) * (31.0 / 63.0)
    assert np.all(rf.candidates(2.5, 2.5) == 2.5)


def test_the_case_list():
    cases = rf.gpu_cases()
    assert [c["name"] for c in cases] == rf.NAMES
    by = {c["name"]: c for c in cases}
    assert sum(len(c["cells"]) for c in cases) <= 320                     # the restatement costs (1 + 3 R) 64 lstsq a cell
    assert len(by["synthetic h100 w2"]["cells"]) == 100 and by["synthetic h100 w2"]["z"].shape == (600, 600)
    c = by["synthetic h15 w0"]
    assert (c["h"], c["w"]) == (15, 0) and 1 < len(c["ages"]) <= 35     # (cut where the cap would be passed: nowhere, at w = 0)
    assert by["h2"]["h"] == 2 and by["h2"]["min_samples"] == 2 and len(by["h2"]["ages"]) == 1
    assert len(by["one age"]["ages"]) == 1 and len(by["64 ages"]["ages"]) == 64 and len(by["no cell"]["cells"]) == 0
    assert 8 * (2 * by["64 ages"]["h"] + 1) * 64 > 65536 and 8 * 2049 * 35 > 65536     # the table in global memory, twice
    assert by["h1024"]["h"] == 1024 and 1 <= len(by["h1024"]["cells"]) <= 8
    assert np.isnan(by["borders, corners and NaN cells"]["z"]).any()


@pytest.mark.parametrize("name", rf.NAMES)
def test_the_restatement_in_two_arithmetics(name):
    """Float64 lstsq per candidate against longdouble Gram-Schmidt per candidate, by the rule of the GPU test (sse_fine and
    the coefficients within RTOL of lstsq at the age that was picked; kt_fine, kt_lo_fine, kt_hi_fine and status_fine equal
    except where the decision lay inside RTOL) and under its cap (such cells at most 1 % of the case): the inputs keep the
    reference itself inside the cap."""
    case = rf.gpu_cases()[rf.NAMES.index(name)]
    for R in rf.LEVELS:
        ref = rf.reference(name, R)
        other = rf.restate(case, R, fit=pr.fit_age_longdouble)
        st = rf.compare(ref, other, case, R)
        print("%s, R = %d: %s" % (name, R, st))
        assert st["fitted"] > 0 or name == "no cell"
        if name == "borders, corners and NaN cells":
            assert st["fitted"] < st["cells"]                              # rows of status 1
            assert sum(r["status"] != 1 and r["n"] < 2 * case["h"] + 1 for r in ref) >= 5       # fitted with points missing
        if name == "best age below the grid":
            assert sum(r["kt_index"] == 0 and r["status_fine"] & 2 for r in ref) > len(ref) // 2
        if name == "best age above the grid":
            assert sum(r["kt_index"] == len(case["ages"]) - 1 and r["status_fine"] & 4 for r in ref) > len(ref) // 2
        if name in ("one age", "h2"):
            assert all(r["kt_fine"] == case["ages"][0] == r["kt_lo_fine"] == r["kt_hi_fine"] and r["status_fine"] == 6
                       for r in ref if r["status"] != 1)


def test_no_level_is_the_grid():
    case = rf.gpu_cases()[0]
    case = dict(case, cells=case["cells"][:5], angle=case["angle"][:5])
    for r in rf.restate(case, 0):
        assert (r["kt_fine"], r["kt_lo_fine"], r["kt_hi_fine"]) == (r["kt"], r["kt_lo"], r["kt_hi"])
        assert (r["a_fine"], r["b_fine"], r["c0_fine"], r["sse_fine"], r["rmse_fine"]) == (r["a"], r["b"], r["c0"], r["sse"], r["rmse"])
        assert r["status_fine"] == r["status"] and r["height_fine"] == 2.0 * r["a"]


# ---- what it recovers (docs/profiles.md, "Continuous ages") -----------------------------------------------------------------
_REC = {}


def recovery(sigma):
    if sigma not in _REC:
        case = rf.recovery_case(sigma)
        _REC[sigma] = (case, rf.restate(case, 2))
    return _REC[sigma]


@pytest.mark.parametrize("sigma", [0.0, 0.05])
def test_recovery_of_an_age_between_two_grid_ages(sigma):
    """synthetic_scarp(600, theta=0.2, kt0=10**1.05), 100 cells on the line, h = 100, w = 2, R = 2.  Measured (also in
    docs/profiles.md): the grid's kt is off by 12.2 % in every cell, with or without noise.  Without noise the median
    |kt_fine / kt0 - 1| is 0.67 % (largest 1.5 %) and [kt_lo_fine, kt_hi_fine] holds kt0 in 79 of 100 cells; at sigma = 0.05
    the median is 2.6 % (largest 8.9 %) and the interval holds kt0 in 54 of 100.  Asserted: what holds by construction."""
    case, rows = recovery(sigma)
    ages = case["ages"]
    assert len(rows) == 100 and all(r["status"] != 1 for r in rows)
    fig = rf.recovery_figures(rows, ages)
    print("sigma %g: %s" % (sigma, fig))
    for r in rows:
        assert r["sse_fine"] <= r["sse"]
        assert ages[0] <= r["kt_lo_fine"] <= r["kt_fine"] <= r["kt_hi_fine"] <= ages[-1]
    if sigma == 0.0:
        assert fig["fine_median"] < fig["grid_median"]
