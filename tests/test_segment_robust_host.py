"""Weights and robust fits of sl.fit_segments (docs/segments.md, "Weights and robust fits"), on the CPU: argument validation
before the library is loaded, the park cap, the layouts of sc_segment_robust_fit and sc_segment_robust_cell, the header's
ABI, the Makefile, the kernels' register budget, the two numpy restatements (tests/segment_robust_reference.py) against
each other on every input of tests/test_gpu_segment_robust.py, and what the feature is for: the trench and the block."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import segment_reference as sr
import segment_robust_reference as qr
from scarplet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FIELDS = ("loss", "scale", "n_down", "ls_index", "n_dormant")
NEW_CELL_FIELDS = ("loss", "n_down", "dormant")


# ---- the arguments are validated before the library is loaded -------------------------------------------------------------
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
    ok = dict(data=g, cells=[3, 77, 78], labels=[1, 2, 2], angle=0.1, half_length=20.0, robust="huber")
    plane = np.ones((40, 50))
    bad = [
        (dict(robust="cauchy"), "a loss that is not built"),
        (dict(robust="Huber"), "the names are lower case"),
        (dict(robust=1), "robust not a string"),
        (dict(robust=True), "robust a bool"),
        (dict(tuning=0.0), "tuning 0"),
        (dict(tuning=-1.0), "tuning < 0"),
        (dict(tuning=np.nan), "tuning NaN"),
        (dict(tuning=np.inf), "tuning inf"),
        (dict(tuning="wide"), "tuning not a number"),
        (dict(tuning=True), "tuning a bool"),
        (dict(iterations=0), "iterations < 1"),
        (dict(iterations=65), "iterations > 64"),
        (dict(iterations=8.0), "iterations not an integer"),
        (dict(iterations=True), "iterations a bool"),
        (dict(robust_scale=0.0), "robust_scale 0"),
        (dict(robust_scale=-0.1), "robust_scale < 0"),
        (dict(robust_scale=np.nan), "robust_scale NaN"),
        (dict(robust_scale=np.inf), "robust_scale inf"),
        (dict(weights=np.ones((40, 51))), "a plane of another shape"),
        (dict(weights=np.ones(2000)), "a plane that is none"),
        (dict(weights=-plane), "weights < 0"),
        (dict(weights=np.where(np.arange(2000).reshape(40, 50) == 7, np.inf, 1.0)), "an infinite weight"),
        (dict(weights="heavy"), "weights not numbers"),
        (dict(max_shift=4.0), "robust with max_shift"),
        (dict(robust=None, weights=plane, max_shift=4.0), "weights with max_shift"),
        (dict(max_width=8.0), "robust with max_width"),
        (dict(max_width=0), "robust with max_width 0"),
        (dict(robust=None, weights=plane, max_width=8.0), "weights with max_width"),
        (dict(robust=None, weights=plane, max_width=8.0, initial_slope=0.6), "weights with max_width and a slope"),
        (dict(robust=None, tuning=2.0), "tuning without robust"),
        (dict(robust=None, robust_scale=0.1), "robust_scale without robust"),
        (dict(robust=None, weights=plane, tuning=2.0), "tuning with weights alone"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError):
            sl.fit_segments(**dict(ok, **kw))
            pytest.fail(what)
    # what is valid gets as far as the device
    for kw in (dict(), dict(robust="tukey"), dict(tuning=2.5), dict(iterations=1), dict(iterations=64), dict(robust_scale=0.3),
               dict(weights=plane), dict(robust=None, weights=plane), dict(weights=np.where(plane > 0, np.nan, 1.0)),
               dict(weights=0 * plane), dict(return_curve=True, return_cells=True), dict(robust=None, iterations=3),
               dict(robust=None), dict(robust=None, max_width=8.0), dict(robust=None, max_shift=2.0), dict(cells=[], labels=[])):
        with pytest.raises(AssertionError, match="the library was asked for"):
            sl.fit_segments(**dict(ok, **kw))


def test_matcher_route_validates():
    import scarplet_amd as sl
    from scarplet_amd import traces

    class Held(object):
        whole, ny, nx, de = True, 40, 50, 2.0

        def result_array(self):
            return [None, None, np.full((40, 50), 0.1)]
    lab = np.zeros((40, 50), dtype=np.int32)
    lab[20, 10:30] = 1
    tr = traces.Traces(lab > 0, lab, None)
    for kw in (dict(robust="cauchy"), dict(robust="huber", tuning=0.0), dict(robust="tukey", iterations=0),
               dict(robust="huber", robust_scale=-1.0), dict(weights=np.ones((4, 5))), dict(robust="huber", max_shift=2.0),
               dict(robust="huber", max_width=8.0), dict(weights=np.ones((40, 50)), max_width=8.0), dict(tuning=2.0)):
        with pytest.raises(ValueError):
            sl.Matcher.fit_segments(Held(), tr, 20.0, **kw)


def test_the_park_cap_counts_nine_planes_and_the_weights(no_library, monkeypatch):
    """8 ((2h + 1)(1 + plane) + 9 A) bytes per cell against SC_SEGMENT_MAX_PARK, a segment at a time: one count, in
    _lib.segment_robust_cap, which the routing and the GPU test of the library's refusal read."""
    import scarplet_amd as sl
    from scarplet_amd import segments
    h, A = 100, 35
    assert _lib.SEGMENT_ROBUST_PLANES == 9
    assert _lib.segment_robust_cap(h, A, False) == (1 << 32) // (8 * (201 + 9 * 35)) == 1040447
    assert _lib.segment_robust_cap(h, A, True) == (1 << 32) // (8 * (402 + 9 * 35)) == 748773
    # a park of 40 cells at h = 10 and two ages without a plane: segments of 40 pass, 41 do not - and pass the plain call
    per = 8 * (21 + 9 * 2)
    monkeypatch.setattr(_lib, "SEGMENT_MAX_PARK", 40 * per)
    g = sl.DEMGrid.from_array(np.zeros((40, 50)), 2.0)
    kw = dict(data=g, angle=0.1, half_length=20.0, ages=[1.0, 2.0])
    with pytest.raises(AssertionError, match="the library was asked for"):
        sl.fit_segments(cells=np.arange(80), labels=np.repeat([1, 2], 40), robust="tukey", **kw)
    with pytest.raises(ValueError, match="a segment of 41 cells: more than 40"):
        sl.fit_segments(cells=np.arange(81), labels=np.repeat([1, 2], [40, 41]), robust="tukey", **kw)
    with pytest.raises(AssertionError, match="the library was asked for"):
        sl.fit_segments(cells=np.arange(81), labels=np.repeat([1, 2], [40, 41]), **kw)
    # the weights are parked beside the profiles: 8 (42 + 18) bytes a cell, 26 cells
    with pytest.raises(ValueError, match="a segment of 27 cells: more than 26"):
        sl.fit_segments(cells=np.arange(27), labels=np.ones(27, dtype=int), weights=np.ones((40, 50)), **kw)
    with pytest.raises(AssertionError, match="the library was asked for"):
        sl.fit_segments(cells=np.arange(26), labels=np.ones(26, dtype=int), weights=np.ones((40, 50)), **kw)
    args = segments.check_args((40, 50), 2.0, np.arange(81), np.repeat([1, 2], [40, 41]), 0.1, 20.0, 0, [1.0, 2.0], 1.0, 4, 1)
    with pytest.raises(ValueError):
        segments.check_robust_park(args, False)


def test_tables_and_defaults():
    import scarplet_amd as sl
    from scarplet_amd import segments
    names = segments.FIT_DTYPE.names
    assert segments.ROBUST_FIT_DTYPE.names == names[:-1] + NEW_FIELDS + ("height",)
    assert segments.ROBUST_FIT_DTYPE.names[:-1] == _lib.SEGMENT_ROBUST_FIT_DTYPE.names
    cn = segments.CELL_DTYPE.names
    assert segments.ROBUST_CELL_DTYPE.names == cn[:-1] + NEW_CELL_FIELDS + ("label",)
    assert segments.ROBUST_CELL_DTYPE.names[2:-1] == _lib.SEGMENT_ROBUST_CELL_DTYPE.names
    for f in (sl.fit_segments, sl.Matcher.fit_segments):
        p = inspect.signature(f).parameters
        assert [p[k].default for k in ("weights", "robust", "tuning", "iterations", "robust_scale")] == [None, None, None, 8, None]
    txt = open(os.path.join(ROOT, "docs", "segments.md")).read()
    assert "## Weights and robust fits" in txt and "Not built: weights" not in txt
    assert "bootstrap_segments" in txt[txt.index("## Weights and robust fits"):]


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_struct_layouts_match_c(tmp_path):
    S, dt = _lib.sc_segment_robust_fit, _lib.SEGMENT_ROBUST_FIT_DTYPE
    C_, cdt = _lib.sc_segment_robust_cell, _lib.SEGMENT_ROBUST_CELL_DTYPE
    names, cnames = [f for f, _ in S._fields_], [f for f, _ in C_._fields_]
    body = '  printf("%zu\\n", sizeof(sc_segment_robust_fit));\n'
    body += "".join('  printf("%%zu\\n", offsetof(sc_segment_robust_fit, %s));\n' % f for f in names)
    body += '  printf("%zu\\n", sizeof(sc_segment_robust_cell));\n'
    body += "".join('  printf("%%zu\\n", offsetof(sc_segment_robust_cell, %s));\n' % f for f in cnames)
    prog = tmp_path / "segrobust.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarplet_hip.h"\nint main(void) {\n' + body
                    + '  printf("%d %lld %d %d %d %d %d %d\\n", SC_SEGMENT_ROBUST_PLANES, SC_SEGMENT_MAX_PARK >> 32, SC_K_COUNT,'
                    ' SC_ABI_VERSION, SC_ROBUST_NONE, SC_ROBUST_HUBER, SC_ROBUST_TUKEY, SC_ROBUST_MAX_ITER);\n  return 0;\n}\n')
    exe = tmp_path / "segrobust"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [ctypes.sizeof(S)] + [getattr(S, f).offset for f in names] + [ctypes.sizeof(C_)] + [getattr(C_, f).offset for f in cnames]
    assert vals == want + [_lib.SEGMENT_ROBUST_PLANES, 1, 11, 10, 0, 1, 2, 64]
    assert ctypes.sizeof(S) == 120 and dt.itemsize == 120 and dt.names == tuple(names)
    assert ctypes.sizeof(C_) == 56 and cdt.itemsize == 56 and cdt.names == tuple(cnames)
    assert [dt.fields[f][1] for f in names] == [getattr(S, f).offset for f in names]
    assert [cdt.fields[f][1] for f in cnames] == [getattr(C_, f).offset for f in cnames]
    # the plain call's row and cell are these structs' heads
    for new, old, extra in ((S, _lib.sc_segment_fit, NEW_FIELDS), (C_, _lib.sc_segment_cell, NEW_CELL_FIELDS)):
        assert new._fields_[:len(old._fields_)] == old._fields_
        assert all(getattr(new, f).offset == getattr(old, f).offset for f, _ in old._fields_)
        assert tuple(f for f, _ in new._fields_[len(old._fields_):]) == extra
    assert (_lib.ROBUST_NONE, _lib.ROBUST_HUBER, _lib.ROBUST_TUKEY, _lib.ROBUST_MAX_ITER) == (0, 1, 2, 64)
    assert len(_lib.K_NAMES) == 11 and _lib.ABI_VERSION == 10


CALLS = ("sc_fit_segments_robust", "sc_fit_segments_robust_dem")


def test_header_declares_the_calls_and_keeps_the_abi():
    txt = open(os.path.join(ROOT, "include", "scarplet_hip.h")).read()
    assert "#define SC_ABI_VERSION 10\n" in txt and _lib.ABI_VERSION == 10
    assert re.search(r"#define\s+SC_K_COUNT\s+11\b", txt) and len(_lib.K_NAMES) == 11
    assert re.search(r"#define\s+SC_SEGMENT_ROBUST_PLANES\s+9\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in CALLS:
        assert re.search(r"\bint %s\s*\(" % n, code), n
    # the call is sc_fit_segments' with weights, loss, tuning, iterations and scale; the _dem form takes (z, ny, nx) ahead
    a, b = _lib.SIGNATURES[CALLS[0]][1], _lib.SIGNATURES[CALLS[1]][1]
    assert len(a) == len(_lib.SIGNATURES["sc_fit_segments"][1]) + 5 and b[:1] + b[4:] == a
    plain, rob = _lib.SIGNATURES["sc_fit_segments"][1], _lib.SIGNATURES["sc_fit_profiles_robust"][1]
    assert a[:16] == plain[:16] and a[16:21] == rob[12:17] and a[21:] == plain[16:]


def test_library_exports_the_calls():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in CALLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert _lib.load().sc_abi_version() == 10


def test_the_makefile_lists_the_source_and_the_build_id_covers_it():
    mk = open(os.path.join(ROOT, "scarplet_amd", "csrc", "Makefile")).read()
    src = re.search(r"^SRC\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "sc_segment_robust.hip" in src and os.path.exists(os.path.join(ROOT, "scarplet_amd", "csrc", "sc_segment_robust.hip"))
    assert re.search(r"^ID_SRC\s*=\s*\$\(SRC\) \$\(HDR\)$", mk, flags=re.M)
    assert "sc_fit.h" in re.search(r"^HDR\s*=\s*(.*)$", mk, flags=re.M).group(1).split()


def test_the_kernels_fit_their_budget():
    from test_isa_budget import kernel_table
    t = kernel_table("sc_segment_robust.hip")
    for stem, count in (("k_sq_partial<", 4), ("k_sq_step<", 8), ("k_sq_loss<", 12), ("k_sq_choose<", 2)):
        assert len([k for k in t if k.startswith(stem)]) == count, (stem, sorted(t))
    for k in ("k_sq_begin", "k_sq_hist", "k_sq_pick"):
        assert k in t, sorted(t)
    for k, r in t.items():
        assert r["scratch"] == 0, (k, r)
        assert r["vgpr"] + r["agpr"] <= 128, (k, r)                        # four waves per SIMD


def test_the_kernels_use_no_inline_assembly():
    for f in ("sc_segment_robust.hip", "sc_fit.h"):
        txt = open(os.path.join(ROOT, "scarplet_amd", "csrc", f)).read()
        assert not re.search(r"\basm\b|__asm", txt), f


# ---- the restatements ---------------------------------------------------------------------------------------------------------
FLOOR = qr.RTOL / 100


def test_the_case_lists():
    h, t = qr.gpu_cases("huber"), qr.gpu_cases("tukey")
    assert list(t) == list(h)[:12] + ["no age survives"] + list(h)[12:] and len(h) == 17
    c = h["sizes 1 2 63 64 65 129"]
    ref = qr.restate(c, fit=qr.joint_fw)
    assert sorted(r["n_profiles"] for r in ref) == [1, 2, 63, 64, 65, 129] and all(r["n_cells"] == r["n_profiles"] + 1 for r in ref)
    assert [r["status"] & 1 for r in qr.restate(h["not fitted"], fit=qr.joint_fw)] == [0, 1, 1]
    assert all(r["status"] == 33 and r["scale"] == 1e-9 for r in qr.restate(t["no age survives"], fit=qr.joint_fw))


@pytest.mark.parametrize("loss", ["huber", "tukey"])
def test_the_two_restatements_agree(loss):
    """float64 lstsq on the full weighted design matrix against the Frisch-Waugh form in longdouble, each run through all the
    iterates on its own, on every input tests/test_gpu_segment_robust.py compares, by compare: their difference is the
    reference's own error and it must stay a hundred times below the tolerance the device is held to.  Measured: loss and
    curve 1.2e-13 (Tukey, "weights: a strip of zeros"), scale 7.2e-14 (the same case), coefficients over the range 2.4e-14
    ("borders"), the largest condition number 245 (h = 31), no index, no n_down and no dormant profile decided differently."""
    worst = {"loss": 0.0, "coef": 0.0, "scale": 0.0, "cond": 0.0, "ties": 0}
    for name, c in qr.gpu_cases(loss).items():
        ref = qr.restate(c)
        ld = qr.restate(c, fit=qr.joint_fw)
        table, ct, curve = qr.tables_of(ld, len(c["cells"]), len(c["ages"]))
        st = qr.compare(c, ref, table, ct, curve)
        print("%-6s %-28s %s" % (loss, name, st))
        for k in worst:
            worst[k] = max(worst[k], st[k])
    print("worst over the cases:", worst)
    assert worst["cond"] <= qr.COND_MAX and worst["ties"] == 0
    assert worst["loss"] <= FLOOR and worst["coef"] <= FLOOR and worst["scale"] <= FLOOR


def test_weights_of_one_and_a_far_constant_are_the_plain_joint_fit():
    c = qr.gpu_cases("huber")["h31"]
    kw = dict(delta=c["delta"], min_samples=c["min_samples"], min_profiles=c["min_profiles"])
    args = (c["de"], c["cells"], c["labels"], c["angle"], c["h"], c["w"], c["ages"])
    plain = sr.fit_segments(c["z"], *args, **kw)
    ones = qr.fit_segments(c["z"], np.ones(c["z"].shape), *args, **kw)
    far = qr.fit_segments(c["z"], None, *args, robust="huber", tuning=1e6, **kw)
    for p, o, f in zip(plain, ones, far):
        assert p["n"] == o["n"] == f["n"] and p["kt_index"] == o["kt_index"] == f["kt_index"] == f["ls_index"]
        assert abs(o["sse"] - p["sse"]) <= 1e-11 * p["sse"] and abs(f["loss"] - p["sse"]) <= 1e-11 * p["sse"]
        assert f["n_down"] == 0 and f["n_dormant"] == 0 and f["scale"] > 0 and np.isnan(o["scale"])


def test_one_profile_is_the_single_profile_restatement():
    import robust_reference as rr
    c = qr.gpu_cases("tukey")["weights: random positive"]
    sa, ca = np.sin(c["angle"]), np.cos(c["angle"])
    for k in range(0, len(c["cells"]), 7):
        one = rr.fit_cell(c["z"], c["weights"], c["de"], c["cells"][k], sa[k], ca[k], c["h"], c["w"], c["ages"], c["delta"],
                          c["min_samples"], fit=rr.wfit_longdouble, **c["robust"])
        seg = qr.fit_segment(c["z"], c["weights"], c["de"], c["cells"][k:k + 1], sa[k:k + 1], ca[k:k + 1], c["h"], c["w"], c["ages"],
                             delta=c["delta"], min_samples=c["min_samples"], fit=qr.joint_fw, **c["robust"])
        for f in ("kt_index", "lo_index", "hi_index", "status", "n_down", "ls_index", "n"):
            assert seg[f] == one[f], (k, f)
        assert np.array_equal(np.isnan(seg["curve"]), np.isnan(one["curve"]))
        for f in ("a", "sse", "loss", "scale", "rmse"):
            assert abs(seg[f] - one[f]) <= 1e-12 * abs(one[f]), (k, f)


# ---- what the feature is for ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", qr.TRENCH_SEEDS)
def test_the_trench(seed):
    """synthetic_scarp(600) with noise 0.05 and a trench of depth 0.8 along the strike, 15 cells from the scarp, on rows
    0..399; 100 cells of the line as ONE segment, h = 100, w = 2, the default 35 ages, T = 8 (the longdouble restatement).
    Least squares: index 8, interval [8, 8].  Huber, Tukey and least squares with the strip masked: index 10, [10, 10]."""
    rows = {}
    for k, kw in (("least squares", {}), ("huber", dict(robust="huber")), ("tukey", dict(robust="tukey")), ("masked", dict(mask=True))):
        rows[k] = qr.restate(qr.trench_case(seed, **kw), fit=qr.joint_fw)[0]
        print(seed, k, rows[k]["kt_index"], rows[k]["lo_index"], rows[k]["hi_index"])
    ls = rows["least squares"]
    assert ls["n_profiles"] == 100 and ls["kt_index"] != qr.TRUE_INDEX
    for k in ("huber", "tukey", "masked"):
        assert (rows[k]["kt_index"], rows[k]["lo_index"], rows[k]["hi_index"]) == (qr.TRUE_INDEX,) * 3, (seed, k)


def test_the_block_leaves_profiles_dormant_under_tukey_alone():
    """+5.0 on rows 200..211 to the right of the scarp: under Tukey the profiles that cross it lose a whole side and go
    dormant at every age (10 or 11 of the 100), under Huber none does, and the age is found either way."""
    for loss in ("huber", "tukey"):
        r = qr.restate(qr.block_case(robust=loss), fit=qr.joint_fw)[0]
        per_age = r["dorm"].sum(axis=1)
        print(loss, r["kt_index"], r["n_dormant"], per_age.min(), per_age.max())
        assert r["kt_index"] == qr.TRUE_INDEX and r["n_profiles"] == 100
        if loss == "tukey":
            assert r["n_dormant"] >= 1 and per_age.min() >= 1 and not np.isnan(r["curve"]).any()
        else:
            assert r["n_dormant"] == 0 and per_age.max() == 0
