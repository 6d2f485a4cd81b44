"""The centre shift of sl.fit_profiles / sl.fit_segments, on the CPU: the numpy restatement (tests/shift_reference.py) on
the offset case of docs/segments.md, argument validation of ``max_shift`` before the library is loaded, the layouts of
sc_profile_shift_fit and sc_segment_shift_cell, the header's ABI, and the kernels' scratch budget."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import profile_reference as pr
import segment_reference as sr
import shift_reference as sh
from scarplet_amd import _lib, _plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGES = _plan.age_grid()
# The offset case as docs/segments.md names it: h = 100, w = 2, D = 8, the default 35 ages (true index 10).  One lstsq
# per (cell, age, shift) and one per age on the 20100 x 301 joint matrix: the fits are shared among the tests below.
H, W, D = 100, 2, 8


def test_shift_order():
    assert sh.shift_order(0) == [0] and sh.shift_order(3) == [0, -1, 1, -2, 2, -3, 3]


_CACHE = {}


def offset_fits(sigma, offsets=True):
    key = (sigma, offsets)
    if key not in _CACHE:
        z, cells, theta, off = sh.offset_case(sigma, offsets)
        _CACHE[key] = (z, cells, theta, off, sh.fit_profiles(z, 1.0, cells, theta, H, W, D, AGES))
    return _CACHE[key]


def test_single_cells_land_on_the_true_age_with_the_shift():
    """Noise-free surface, cells up to six columns off the line: every single-cell fit lands on index 10 with the
    shift, fewer than half do without; the shift found is the offset seen along the profile."""
    z, cells, theta, off, rows = offset_fits(0.0)
    assert len(cells) == 100 and off.min() == -6 and off.max() == 6
    with_shift = np.array([r["kt_index"] for r in rows])
    without = np.array([r["kt_index"] for r in pr.fit_profiles(z, 1.0, cells, theta, H, W, AGES)])
    d = np.array([r["shift_index"] for r in rows])
    print("on index 10: %d of 100 without the shift, %d with; |d + offset cos(theta)| at most %.3f"
          % ((without == 10).sum(), (with_shift == 10).sum(), np.abs(d + off * np.cos(theta)).max()))
    assert (with_shift == 10).all()
    assert (without == 10).sum() < 50
    assert np.abs(d + off * np.cos(theta)).max() <= 1.5
    assert np.abs(d).max() < D and not any(r["status"] & 8 for r in rows)    # no fit ran into the end of its range
    assert all(r["dof"] == r["n"] - 4 for r in rows)


def joint(z, cells, theta, shifts):
    lab = np.ones(len(cells), dtype=int)
    return sh.fit_segments(z, 1.0, cells, lab, theta, H, W, D, AGES, shifts)[0]


def test_joint_fit_is_two_steps_too_old_without_the_shift_and_right_with_it():
    z, cells, theta, off, rows = offset_fits(0.5)
    without = sr.fit_segments(z, 1.0, cells, np.ones(100, dtype=int), theta, H, W, AGES)[0]
    row = joint(z, cells, theta, np.array([r["shifts"] for r in rows]))
    print("joint fit: index %d [%d, %d] without the shift; %d [%d, %d] with, a %.5f, condition number %.1f"
          % (without["kt_index"], without["lo_index"], without["hi_index"], row["kt_index"],
             row["lo_index"], row["hi_index"], row["a"], row["cond"]))
    assert (without["kt_index"], without["lo_index"], without["hi_index"]) == (12, 12, 12)
    assert (row["kt_index"], row["lo_index"], row["hi_index"]) == (10, 10, 10)
    assert abs(row["a"] - 1.0037) <= 1e-4
    assert row["n_profiles"] == 100 and row["dof"] == row["n"] - 3 * 100 - 1 and not row["status"] & 8
    assert row["cond"] <= pr.COND_MAX
    d = row["du"][:, row["kt_index"]]
    assert np.abs(d + off * np.cos(theta)).max() <= 1.5


def test_no_offsets_the_shift_does_no_harm():
    z, cells, theta, off, rows = offset_fits(0.5, offsets=False)
    assert not off.any()
    row = joint(z, cells, theta, np.array([r["shifts"] for r in rows]))
    assert row["kt_index"] == 10


def test_one_profile_segment_is_the_shifted_single_fit():
    z, cells, theta, off, rows = offset_fits(0.5)
    for k in (0, 17):
        seg = sh.fit_segments(z, 1.0, cells[k:k + 1], [3], theta, H, W, D, AGES, rows[k]["shifts"][None, :])[0]
        one = rows[k]
        assert seg["dof"] == one["dof"] == one["n"] - 4
        assert (seg["kt_index"], seg["lo_index"], seg["hi_index"], seg["status"]) == \
            (one["kt_index"], one["lo_index"], one["hi_index"], one["status"])
        assert abs(seg["a"] - one["a"]) <= 1e-10 and abs(seg["sse"] - one["sse"]) <= 1e-10 * one["sse"]


def test_zero_range_is_the_unshifted_restatement():
    z, cells, theta, off = sh.offset_case(0.5)
    a = sh.fit_profiles(z, 1.0, cells[:3], theta, 40, 1, 0, AGES[:12])
    b = pr.fit_profiles(z, 1.0, cells[:3], theta, 40, 1, AGES[:12])
    for x, y in zip(a, b):
        assert x["dof"] == y["n"] - 3 and x["shift_index"] == 0 and x["shift"] == 0.0
        for f in ("n", "kt_index", "lo_index", "hi_index", "status", "a", "b", "c0", "sse", "rmse"):
            assert x[f] == y[f], f


# ---- max_shift is validated before the library is loaded -------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    import scarplet_amd.core as core

    def refuse(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(core, "_context", refuse)
    monkeypatch.setattr(_lib, "load", refuse)


def test_max_shift_validates_before_the_library_is_loaded(no_library):
    import scarplet_amd as sl
    g = sl.DEMGrid.from_array(np.zeros((40, 50)), 2.0)
    okp = dict(data=g, cells=[3, 77], angle=0.1, half_length=20.0)                 # h = 10, min_samples = 4
    oks = dict(okp, labels=[1, 1])
    bad = [
        (dict(max_shift=-1.0), "max_shift < 0"),
        (dict(max_shift=np.nan), "max_shift NaN"),
        (dict(max_shift=np.inf), "max_shift inf"),
        (dict(max_shift="far"), "max_shift not a number"),
        (dict(max_shift=True), "max_shift a bool"),
        (dict(max_shift=14.0), "7 cells, more than h - min_samples = 6"),
        (dict(max_shift=12.0, min_samples=5), "6 cells, more than h - min_samples = 5"),
        (dict(max_shift=2.0 * 65, half_length=400.0), "65 cells, more than 64"),
        (dict(return_shift=True), "return_shift without max_shift"),
        (dict(max_shift=None, return_shift=True), "return_shift with max_shift None"),
    ]
    for fn, ok in ((sl.fit_profiles, okp), (sl.fit_segments, oks)):
        for kw, what in bad:
            with pytest.raises(ValueError):
                fn(**dict(ok, **kw))
                pytest.fail(what)
        # what is valid gets as far as the device: the whole range, the largest shift the call takes, zero
        for kw in (dict(max_shift=13.9), dict(max_shift=2.0 * 64, half_length=400.0), dict(max_shift=0),
                   dict(max_shift=0.0, return_shift=True), dict()):
            with pytest.raises(AssertionError, match="the library was asked for"):
                fn(**dict(ok, **kw))


def test_check_shift_floors_to_cells():
    from scarplet_amd import profiles
    assert profiles.check_shift(None, False, 2.0, 10, 4) is None
    assert profiles.check_shift(0, False, 2.0, 10, 4) == 0
    assert profiles.check_shift(5.9, True, 2.0, 10, 4) == 2
    assert profiles.check_shift(12.0, False, 2.0, 10, 4) == 6


def test_matcher_routes_validate_max_shift():
    import scarplet_amd as sl
    from scarplet_amd import traces

    class Held(object):
        whole, ny, nx, de = True, 40, 50, 2.0
    tr = traces.Traces(np.zeros((40, 50), dtype=bool), np.zeros((40, 50), dtype=np.int32),
                       traces._table(np.zeros(0, dtype=_lib.SEGMENT_DTYPE)))
    for kw in (dict(max_shift=-1.0), dict(max_shift=14.0), dict(return_shift=True)):
        with pytest.raises(ValueError, match="shift"):
            sl.Matcher.fit_profiles(Held(), [3, 77], 20.0, angle=0.1, **kw)
        with pytest.raises(ValueError, match="shift"):
            sl.Matcher.fit_segments(Held(), tr, 20.0, strike="segment", **kw)


def test_tables_with_the_shift():
    from scarplet_amd import profiles, segments
    assert profiles.SHIFT_FIT_DTYPE.names == profiles.FIT_DTYPE.names + ("shift_index", "shift")
    assert segments.SHIFT_CELL_DTYPE.names == ("row", "col", "cell", "used", "n", "b", "c0", "sse", "shift_index", "shift",
                                               "label")


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_shift_struct_layouts_match_c(tmp_path):
    structs = [("sc_profile_shift_fit", _lib.sc_profile_shift_fit, _lib.PROFILE_SHIFT_DTYPE),
               ("sc_segment_shift_cell", _lib.sc_segment_shift_cell, _lib.SEGMENT_SHIFT_CELL_DTYPE)]
    body = ""
    for cname, S, _ in structs:
        body += '  printf("%%zu\\n", sizeof(%s));\n' % cname
        body += "".join('  printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f) for f, _ in S._fields_)
    prog = tmp_path / "shift.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarplet_hip.h"\nint main(void) {\n' + body
                    + '  printf("%d %d %d\\n", SC_PROFILE_MAX_SHIFT, SC_K_COUNT, SC_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "shift"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = []
    for _, S, dt in structs:
        names = [f for f, _ in S._fields_]
        want += [ctypes.sizeof(S)] + [getattr(S, f).offset for f in names]
        assert dt.itemsize == ctypes.sizeof(S) and dt.names == tuple(names)
        assert [dt.fields[f][1] for f in names] == [getattr(S, f).offset for f in names]
    assert vals == want + [_lib.PROFILE_MAX_SHIFT, len(_lib.K_NAMES), 10]    # no new timing slot, the ABI as it was
    # the shared fields sit where sc_profile_fit / sc_segment_cell have them
    for S, T in ((_lib.sc_profile_shift_fit, _lib.sc_profile_fit), (_lib.sc_segment_shift_cell, _lib.sc_segment_cell)):
        assert S._fields_[:len(T._fields_)] == T._fields_
        assert all(getattr(S, f).offset == getattr(T, f).offset for f, _ in T._fields_)
    assert [f for f, _ in _lib.sc_profile_shift_fit._fields_][-2:] == ["shift_index", "shift"]
    assert [f for f, _ in _lib.sc_segment_shift_cell._fields_][-1] == "shift_index"


SHIFT_CALLS = ("sc_fit_profiles_shift", "sc_fit_profiles_shift_dem", "sc_fit_segments_shift", "sc_fit_segments_shift_dem")


def test_header_still_says_abi_10_and_declares_the_shift_calls():
    txt = open(os.path.join(ROOT, "include", "scarplet_hip.h")).read()
    assert "#define SC_ABI_VERSION 10\n" in txt and _lib.ABI_VERSION == 10
    assert re.search(r"#define\s+SC_K_COUNT\s+11\b", txt) and len(_lib.K_NAMES) == 11
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in SHIFT_CALLS:
        assert re.search(r"\bint %s\s*\(" % n, code), n


def test_library_exports_the_shift_calls():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in SHIFT_CALLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert _lib.load().sc_abi_version() == 10


def test_shift_kernels_have_no_scratch():
    from test_isa_budget import kernel_table
    t = dict(kernel_table("sc_profile.hip"), **kernel_table("sc_segment.hip"))
    # (k_sg_resid and k_sg_choose serve the calls with and without a shift)
    for k in ("k_pf_shift<true>", "k_pf_shift<false>", "k_sg_shift<true>", "k_sg_shift<false>", "k_sg_resid<true>",
              "k_sg_resid<false>", "k_sg_choose<sc_segment_shift_cell>"):
        assert k in t, sorted(t)
        assert t[k]["scratch"] == 0, (k, t[k])
        assert t[k]["vgpr"] + t[k]["agpr"] <= 128, (k, t[k])               # four waves per SIMD
