"""The initial slope of sl.fit_profiles (docs/profiles.md, "The initial slope"), on the CPU: argument validation of
``max_width``, ``initial_slope`` and ``return_width`` before the library is loaded, the layout of sc_profile_ramp_fit, the
header's ABI, the kernels' scratch budget, the two numpy restatements (tests/ramp_reference.py) against each other on
every input of tests/test_gpu_ramp.py, the condition cap of those inputs, and what the model recovers on a 2-D surface."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.special import erf

import profile_reference as pr
import ramp_reference as rr
from scarplet_amd import _lib, _plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGES = _plan.age_grid()


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
    ok = dict(data=g, cells=[3, 77], angle=0.1, half_length=20.0)                  # h = 10, min_samples = 4
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
        (dict(max_width=8.0, weights=np.ones((40, 50))), "with weights"),
        (dict(max_width=8.0, robust="huber"), "with robust"),
        (dict(max_width=0, robust="tukey"), "max_width 0 with robust"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError):
            sl.fit_profiles(**dict(ok, **kw))
            pytest.fail(what)
    # what is valid gets as far as the device: the whole range, the largest width the call takes, zero, both modes
    for kw in (dict(max_width=13.9), dict(max_width=2.0 * 64, half_length=400.0), dict(max_width=0),
               dict(max_width=0.0, return_width=True), dict(max_width=2.0, initial_slope=0.6),
               dict(max_width=12.0, initial_slope=1e-3, return_width=True, return_curve=True), dict()):
        with pytest.raises(AssertionError, match="the library was asked for"):
            sl.fit_profiles(**dict(ok, **kw))


def test_check_width_floors_to_cells():
    from scarplet_amd import profiles
    assert profiles.check_width(None, None, False, 2.0, 10, 4) is None
    assert profiles.check_width(0, None, False, 2.0, 10, 4) == (0, _lib.RAMP_FREE, 0.0)
    assert profiles.check_width(5.9, None, True, 2.0, 10, 4) == (2, _lib.RAMP_FREE, 0.0)
    assert profiles.check_width(12.0, 0.6, False, 2.0, 10, 4) == (6, _lib.RAMP_SLOPE, 0.6)
    assert (_lib.RAMP_FREE, _lib.RAMP_SLOPE, _lib.PROFILE_MAX_WIDTH) == (0, 1, 64)


def test_matcher_route_validates_max_width():
    import scarplet_amd as sl

    class Held(object):
        whole, ny, nx, de = True, 40, 50, 2.0
    for kw in (dict(max_width=-1.0), dict(max_width=14.0), dict(return_width=True), dict(initial_slope=0.6),
               dict(max_width=8.0, initial_slope=-1.0), dict(max_width=8.0, max_shift=2.0), dict(max_width=8.0, robust="huber")):
        with pytest.raises(ValueError, match="width|slope"):
            sl.Matcher.fit_profiles(Held(), [3, 77], 20.0, angle=0.1, **kw)


def test_table_with_the_width():
    from scarplet_amd import profiles
    assert profiles.RAMP_FIT_DTYPE.names == profiles.FIT_DTYPE.names + ("width_index", "width", "initial_slope")
    rows = np.zeros(2, dtype=_lib.PROFILE_RAMP_DTYPE)
    rows["cell"], rows["a"] = [7, 53], [0.5, -1.0]
    t = profiles._table(rows, 50, label=[3, 3])
    assert t.dtype.names == profiles.RAMP_FIT_DTYPE.names + ("label",)
    assert list(t["row"]) == [0, 1] and list(t["col"]) == [7, 3] and list(t["height"]) == [1.0, -2.0]


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_ramp_struct_layout_matches_c(tmp_path):
    S, dt = _lib.sc_profile_ramp_fit, _lib.PROFILE_RAMP_DTYPE
    names = [f for f, _ in S._fields_]
    body = '  printf("%zu\\n", sizeof(sc_profile_ramp_fit));\n'
    body += "".join('  printf("%%zu\\n", offsetof(sc_profile_ramp_fit, %s));\n' % f for f in names)
    prog = tmp_path / "ramp.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarplet_hip.h"\nint main(void) {\n' + body
                    + '  printf("%d %d %d %d %d\\n", SC_PROFILE_MAX_WIDTH, SC_RAMP_FREE, SC_RAMP_SLOPE, SC_K_COUNT, SC_ABI_VERSION);\n'
                    + '  return 0;\n}\n')
    exe = tmp_path / "ramp"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [ctypes.sizeof(S)] + [getattr(S, f).offset for f in names]
    assert dt.itemsize == ctypes.sizeof(S) and dt.names == tuple(names)
    assert [dt.fields[f][1] for f in names] == [getattr(S, f).offset for f in names]
    # no new timing slot, the ABI as it was
    assert vals == want + [_lib.PROFILE_MAX_WIDTH, _lib.RAMP_FREE, _lib.RAMP_SLOPE, len(_lib.K_NAMES), 10]
    # the shared fields sit where sc_profile_fit has them, and the struct is sc_profile_shift_fit with three fields for two
    T = _lib.sc_profile_fit
    assert S._fields_[:len(T._fields_)] == T._fields_
    assert all(getattr(S, f).offset == getattr(T, f).offset for f, _ in T._fields_)
    assert names[-3:] == ["width_index", "width", "initial_slope"]
    assert S.width_index.offset == _lib.sc_profile_shift_fit.shift_index.offset
    assert S.width.offset == _lib.sc_profile_shift_fit.shift.offset


RAMP_CALLS = ("sc_fit_profiles_ramp", "sc_fit_profiles_ramp_dem")


def test_header_still_says_abi_10_and_declares_the_ramp_calls():
    txt = open(os.path.join(ROOT, "include", "scarplet_hip.h")).read()
    assert "#define SC_ABI_VERSION 10\n" in txt and _lib.ABI_VERSION == 10
    assert re.search(r"#define\s+SC_K_COUNT\s+11\b", txt) and len(_lib.K_NAMES) == 11
    assert re.search(r"#define\s+SC_PROFILE_MAX_WIDTH\s+64\b", txt)
    assert re.search(r"#define\s+SC_RAMP_FREE\s+0\b", txt) and re.search(r"#define\s+SC_RAMP_SLOPE\s+1\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in RAMP_CALLS:
        assert re.search(r"\bint %s\s*\(" % n, code), n


def test_library_exports_the_ramp_calls():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in RAMP_CALLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    # the _dem form takes (z, ny, nx) ahead of the same arguments
    a, b = _lib.SIGNATURES["sc_fit_profiles_ramp"][1], _lib.SIGNATURES["sc_fit_profiles_ramp_dem"][1]
    assert len(a) == 18 and b[:1] + b[4:] == a
    assert _lib.load().sc_abi_version() == 10


def test_ramp_kernels_have_no_scratch():
    from test_isa_budget import kernel_table
    t = kernel_table("sc_ramp.hip")
    for k in ("k_pf_ramp<true>", "k_pf_ramp<false>"):
        assert k in t, sorted(t)
        assert t[k]["scratch"] == 0, (k, t[k])
        assert t[k]["vgpr"] + t[k]["agpr"] <= 128, (k, t[k])               # four waves per SIMD
    assert t["k_rp_table"]["scratch"] == 0


# ---- the restatements ---------------------------------------------------------------------------------------------------------
def test_longdouble_erf_is_the_erf():
    x = np.linspace(-9.0, 9.0, 1801)
    assert np.abs(rr.erf_longdouble(x).astype(np.float64) - erf(x)).max() <= 2.3e-16
    assert rr.erf_longdouble(np.longdouble(0)) == 0 and rr.erf_longdouble(np.longdouble(-8)) == -1


def test_the_column_tends_to_the_erf_and_f_differentiates_to_it():
    """g -> erf(s / (2 sqrt(kt))) as L -> 0, and F' = erf: the central difference of the table at one cell is the erf up
    to de^2 F''' / 6."""
    s = np.arange(-100, 101).astype(np.float64)
    for kt in (1.0, 10.0, 316.0):
        e = erf(s / (2 * np.sqrt(kt)))
        assert np.abs(rr.g_exact(s, kt, 1e-3) - e).max() <= 1e-7
        third = 0.25 / kt                      # |F'''| = |erf''| is at most exp(-1/2) / (kt sqrt(2 pi)) = 0.242 / kt, at s = sqrt(2 kt)
        E = rr.columns(np.arange(-100, 101), 100, 1, 1.0, [kt], *rr._tables(100, 1, 1.0, [kt]))
        assert np.array_equal(E[0, 0], e)
        assert np.abs(E[0, 1] - e).max() <= third / 6


def test_the_case_list():
    cases = rr.gpu_cases()
    assert [c["name"] for c in cases] == rr.NAMES
    for c in cases:
        assert 0 <= c["M"] <= min(_lib.PROFILE_MAX_WIDTH, c["h"] - c["min_samples"]) and len(c["cells"]) <= 500
        assert max(c["z"].shape) <= 600
    by = {c["name"]: c for c in cases}
    assert {(by[n]["h"], by[n]["w"], by[n]["M"]) for n in rr.NAMES[:3]} == {(100, 0, 8), (100, 5, 1), (30, 5, 4)}
    c = by["h100 w0 M8"]
    assert len(c["ages"]) * (c["M"] + 1) == 315                                # five rounds, the last one partial
    assert 8 * (2 * (c["h"] + c["M"]) + 1) * len(c["ages"]) <= 65536            # the table in LDS
    c = by["64 ages M1"]
    assert len(c["ages"]) == 64 and 8 * (2 * (c["h"] + c["M"]) + 1) * 64 > 65536  # ... and in global memory
    assert len(by["one age M8"]["ages"]) == 1 and by["one age M8"]["M"] == 8
    c = by["M = h - min_samples"]
    assert c["M"] == c["h"] - c["min_samples"]
    assert by["de 2"]["de"] == 2.0 and len(by["no cell"]["cells"]) == 0
    assert by["dof < 1"]["slope"] is None and all(by[n]["slope"] > 0 for n in rr.NAMES[:-1])


@pytest.mark.parametrize("name", rr.NAMES)
def test_the_two_restatements_agree(name):
    """Float64 lstsq on equilibrated columns against longdouble Gram-Schmidt on a longdouble table, on every input of the
    GPU tests: RTOL / 100 in every sse_im and every coefficient (relative to the profile's range), every compared pair
    under the condition cap, and no m_i, no index and no status decided differently in either mode.  The subtraction
    F(s + L) - F(s - L) does cost the float64 restatement: under the condition cap alone it misses this bound, 9.4e-10 in
    the coefficients (2.2e-11 in the sse) at h = 12, M = 8 with 32 ages and 1.6e-11 at h = 30, M = 4 with all 35
    (docs/profiles.md, "The initial slope").  The age grids of the cases are therefore cut to where it holds
    (ramp_reference.NA); measured on them, over all cases: 2.7e-13 in the sse and 1.2e-12 in the coefficients."""
    case = {c["name"]: c for c in rr.gpu_cases()}[name]
    a, b = rr.case_pairs(case), rr.case_pairs(case, longdouble=True)
    worst = {"sse": 0.0, "coef": 0.0, "cond": 0.0, "usable": 0}
    scale = np.array([1.0, case["h"] * case["de"], 1.0])
    for x, y in zip(a, b):
        assert x["n"] == y["n"] and x["usable"] == y["usable"]
        if not x["usable"]:
            continue
        worst["usable"] += 1
        assert x["cond"] <= rr.COND_MAX, (x["cell"], x["cond"])
        gy = y["grid"].astype(np.float64)
        worst["sse"] = max(worst["sse"], float(np.max(np.abs(x["grid"] - gy) / gy)))
        worst["coef"] = max(worst["coef"], float(np.max(np.abs(x["coefs"] - y["coefs"].astype(np.float64)) * scale)) / x["ptp"])
        worst["cond"] = max(worst["cond"], x["cond"])
    print("%s: %s" % (name, worst))
    assert worst["sse"] <= rr.RTOL / 100 and worst["coef"] <= rr.RTOL / 100, worst
    for mode in (rr.FREE, rr.SLOPE):
        if mode == rr.SLOPE and case["slope"] is None:
            continue
        for x, y in zip(rr.restate(case, mode), rr.restate(case, mode, longdouble=True)):
            for f in ("n", "dof", "kt_index", "lo_index", "hi_index", "status", "width_index"):
                assert x[f] == y[f], (name, mode, x["cell"], f, x[f], y[f])
            assert np.array_equal(x["widths"], y["widths"]), (name, mode, x["cell"])


def test_the_dof_case_has_the_cell_it_is_about():
    case = {c["name"]: c for c in rr.gpu_cases()}["dof < 1"]
    rows = rr.restate(case, rr.FREE)
    assert rows[0]["usable"] and rows[0]["n"] == 4 and rows[0]["dof"] == 0 and rows[0]["status"] == 1
    assert all(r["n"] == 7 and r["dof"] == 3 and r["status"] != 1 for r in rows[1:])
    # ... and with the slope given the constraint fixes the width: the same cell has a degree of freedom
    assert rr.choose_cell(rr.case_pairs(case)[0], 1.0, 1, case["ages"], rr.SLOPE, 0.5)["dof"] == 1


def test_width_zero_is_the_plain_restatement():
    case = {c["name"]: c for c in rr.gpu_cases()}["h30 w5 M4"]
    plain = pr.fit_profiles(case["z"], 1.0, case["cells"][:6], case["angle"][:6], 30, 5, case["ages"], 1.0, 15)
    zero = rr.fit_profiles(case["z"], 1.0, case["cells"][:6], case["angle"][:6], 30, 5, 0, case["ages"], min_samples=15)
    for x, y in zip(zero, plain):
        assert x["dof"] == y["n"] - 3 and x["width_index"] == 0 and x["width"] == 0.0 and np.isinf(x["initial_slope"])
        for f in ("n", "kt_index", "lo_index", "hi_index", "status"):
            assert x[f] == y[f], f
        assert abs(x["sse"] - y["sse"]) <= 1e-11 * y["sse"] and abs(x["a"] - y["a"]) <= 1e-11


# ---- what it does: the recovery surface of docs/profiles.md ---------------------------------------------------------------------
_REC = {}


def recovery(noise):
    if noise not in _REC:
        z, cells, theta, ages = rr.recovery_case(noise)
        R = rr.REC
        _REC[noise] = (z, cells, theta, ages, rr.pairs_of_cells(z, 1.0, cells, theta, R["h"], R["w"], R["M"], ages))
    return _REC[noise]


def test_the_given_slope_finds_the_age_the_plain_model_misses():
    """600 x 600, theta = 0.2, a ramp of half-width 6 cells diffused for ages[10], noise 0.02, 100 cells on the line, h = 100,
    w = 2.  Measured: the true age in 100 of 100 cells with initial_slope = |b + a / L|, in 0 of 100 with the plain model
    (index 12 in all of them, every interval one age wide)."""
    R = rr.REC
    z, cells, theta, ages, pairs = recovery(R["noise"])
    assert len(cells) == 100
    given = rr.fit_profiles(z, 1.0, cells, theta, R["h"], R["w"], R["M"], ages, mode=rr.SLOPE, slope=R["slope"], pairs=pairs)
    plain = pr.fit_profiles(z, 1.0, cells, theta, R["h"], R["w"], ages)
    hit = sum(r["kt_index"] == R["index"] for r in given)
    miss = sum(r["kt_index"] == R["index"] for r in plain)
    print("true age: %d of 100 with the slope given, %d of 100 with the plain model (its indices: %s)"
          % (hit, miss, sorted(set(r["kt_index"] for r in plain))))
    assert hit >= 90
    assert miss <= 10
    assert max(r["cond"] for r in given) <= rr.COND_MAX
    assert all(r["dof"] == r["n"] - 3 for r in given) and not any(r["status"] & 8 for r in given)


def test_the_free_width_finds_age_and_width_without_noise():
    R = rr.REC
    z, cells, theta, ages, pairs = recovery(0.0)
    free = rr.fit_profiles(z, 1.0, cells, theta, R["h"], R["w"], R["M"], ages, pairs=pairs)
    assert all(r["width_index"] == R["L"] and r["kt_index"] == R["index"] for r in free)
    assert all(r["dof"] == r["n"] - 4 and r["status"] == 0 for r in free)
    # the slope it reports is the planted one
    assert max(abs(r["initial_slope"] - (-0.01 + 1.0 / 6.0)) for r in free) <= 2e-3


def test_the_free_width_under_noise_widens_its_interval():
    """One profile identifies (age, width) poorly - a ramp of half-width L looks like a step older by L^2 / 6 - and the
    interval says so.  Measured at noise 0.02: the true age in 73 of 100 cells, the mean interval 1.12 ages where the
    plain model claims 1.0 around the wrong age."""
    R = rr.REC
    z, cells, theta, ages, pairs = recovery(R["noise"])
    free = rr.fit_profiles(z, 1.0, cells, theta, R["h"], R["w"], R["M"], ages, pairs=pairs)
    plain = pr.fit_profiles(z, 1.0, cells, theta, R["h"], R["w"], ages)
    width = lambda rows: float(np.mean([r["hi_index"] - r["lo_index"] + 1 for r in rows]))
    hit = sum(r["kt_index"] == R["index"] for r in free)
    print("width free: the true age in %d of 100, mean interval %.2f ages (plain: %.2f)" % (hit, width(free), width(plain)))
    assert hit > sum(r["kt_index"] == R["index"] for r in plain)
    assert width(free) >= width(plain)
