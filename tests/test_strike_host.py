"""sl.fit_along_strike on the CPU: the stations and windows against hand-computed values, argument validation before the
library is loaded, the layout of sc_strike_fit and the header's ABI, the exported symbols, the kernels' register budget,
and the numpy restatement (tests/strike_reference.py) on the noisy case of docs/segments.md."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import segment_reference as sr
import strike_reference as stk
from scarplet_amd import _lib, _plan, strike

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGES = _plan.age_grid()


def handover(shape, de, cells, labels, angle, window, step=None):
    a, where = strike.check_args(shape, de, cells, labels, angle, 10.0 * de, 0, window, step, AGES, 1.0, 4, 1, None)
    out = dict(zip(("cells", "sa", "ca", "seg_start", "seg_label", "seg_win_start", "win_lo", "win_hi"), a[:8]))
    out.update(zip(("t", "row", "col"), where))
    return out


# ---- stations and windows ------------------------------------------------------------------------------------------------
def test_windows_on_a_vertical_line():
    """Strike 0: t = de row.  Twenty cells of one column at de = 2, rows 10..29: t = 20..58, span 38.  Window 12, step 6:
    ns = floor(38 / 6) + 1 = 7, the first centre 20 + (38 - 36) / 2 = 21, then 27, 33, ... 57; the window of u holds the
    rows with |2 row - u| <= 6."""
    nx = 50
    rows = np.arange(10, 30)
    perm = np.random.default_rng(1).permutation(20)
    cells = (rows * nx + 7)[perm]
    h = handover((60, nx), 2.0, cells, np.full(20, 4), 0.0, 12.0)          # step: window / 2
    assert h["seg_label"].tolist() == [4] and h["seg_start"].tolist() == [0, 20] and h["seg_win_start"].tolist() == [0, 7]
    assert (h["cells"] // nx).tolist() == rows.tolist()                    # sorted along the strike
    assert h["t"].tolist() == [21.0, 27.0, 33.0, 39.0, 45.0, 51.0, 57.0]
    # u = 21: rows 7.5..13.5 -> 10..13; u = 27: 10.5..16.5 -> 11..16; ... u = 57: 25.5..31.5 -> 26..29
    assert h["win_lo"].tolist() == [0, 1, 4, 7, 10, 13, 16] and h["win_hi"].tolist() == [4, 7, 10, 13, 16, 19, 20]
    assert h["row"].tolist() == [11.5, 13.5, 16.5, 19.5, 22.5, 25.5, 27.5] and (h["col"] == 7.0).all()
    # window 10 at step 10: ns = 4, first centre 20 + (38 - 30) / 2 = 24: rows 9.5..14.5, 14.5..19.5, ...
    h = handover((60, nx), 2.0, cells, np.full(20, 4), 0.0, 10.0, 10.0)
    assert h["t"].tolist() == [24.0, 34.0, 44.0, 54.0] and h["win_lo"].tolist() == [0, 5, 10, 15] and h["win_hi"].tolist() == [5, 10, 15, 20]
    h = handover((60, nx), 2.0, cells, np.full(20, 4), 0.0, 4.0, 4.0)
    # ns = 10, first centre 20 + (38 - 36) / 2 = 21: |2 row - 21| <= 2 -> rows 10 and 11, then 12 and 13, ...
    assert h["t"][0] == 21.0 and h["win_lo"].tolist() == list(range(0, 20, 2)) and h["win_hi"].tolist() == list(range(2, 22, 2))
    # equal t keeps the input order: rows 10, 6, 10, 10 of two columns at the same t
    h = handover((60, nx), 2.0, [507, 307, 508, 506], [1, 1, 1, 1], 0.0, 2.0, 2.0)
    assert h["cells"].tolist() == [307, 507, 508, 506]
    # span 8, ns = 5, centres 12, 14, ... 20: |t - u| <= 1
    assert h["t"].tolist() == [12.0, 14.0, 16.0, 18.0, 20.0]
    assert h["win_lo"].tolist() == [0, 1, 1, 1, 1] and h["win_hi"].tolist() == [1, 1, 1, 1, 4]
    ref = stk.handover(np.array([507, 307, 508, 506]), np.ones(4, dtype=int), np.zeros(4), nx, 2.0)
    assert ref[0][1].tolist() == [1, 0, 2, 3]


def test_windows_on_a_diagonal():
    """Strike pi / 4, cells (r, r), r = 5..24 at de = 1: t = r sqrt(2), span 19 sqrt(2) = 26.87.  Window 6, step 3:
    ns = floor(26.87 / 3) + 1 = 9, the first centre 5 sqrt(2) + (19 sqrt(2) - 24) / 2."""
    nx = 40
    r = np.arange(5, 25)
    cells = r * nx + r
    h = handover((40, nx), 1.0, cells, np.ones(20, dtype=int), np.pi / 4, 6.0)
    q = math.sqrt(2.0)
    first = 5 * q + (19 * q - 24) / 2
    assert len(h["t"]) == 9 and np.allclose(h["t"], first + 3.0 * np.arange(9), rtol=0, atol=1e-12)
    want = [[v for v in r if abs(v * q - (first + 3 * k)) <= 3.0] for k in range(9)]
    assert h["win_lo"].tolist() == [w[0] - 5 for w in want] and h["win_hi"].tolist() == [w[-1] - 5 + 1 for w in want]
    # by hand: the first centre is 8.506, its window 5.506..11.506 holds r sqrt(2) = 7.07, 8.49, 9.90, 11.31 (r = 5..8) and
    # not 12.73; a step of 3 is 2.12 cells: the next holds r = 7..10 (9.90 .. 14.14 in 8.506..14.506), and so on
    assert want[0] == [5, 6, 7, 8] and want[1] == [7, 8, 9, 10] and want[8] == [21, 22, 23, 24]
    assert [w[0] for w in want] == [5, 7, 9, 11, 13, 15, 17, 19, 21] and all(len(w) == 4 for w in want)
    assert np.allclose(h["row"], [np.mean(w) for w in want]) and np.array_equal(h["row"], h["col"])
    # two segments, interleaved, the second with a hole along it: its stations go on across the hole, their windows empty
    lab = np.where(np.arange(20) % 2 == 0, 2, 1)
    cells2 = cells.copy()
    cells2[lab == 1] = np.array([5, 6, 7, 30, 31, 32, 33, 34, 35, 36]) * nx + 3      # a vertical line with a hole of 22 rows
    ang = np.where(lab == 1, 0.0, np.pi / 4)
    h = handover((40, nx), 1.0, cells2, lab, ang, 4.0, 4.0)
    assert h["seg_label"].tolist() == [1, 2] and h["seg_start"].tolist() == [0, 10, 20]
    # label 1: t = 5..36, span 31, ns = 8, first centre 5 + (31 - 28) / 2 = 6.5: rows 4.5..8.5 | 8.5..12.5 (none) ...
    # 28.5..32.5 | 32.5..36.5
    s1 = slice(0, h["seg_win_start"][1])
    assert h["seg_win_start"][1] == 8 and h["t"][s1].tolist() == [6.5 + 4 * k for k in range(8)]
    assert h["win_lo"][s1].tolist() == [0, 3, 3, 3, 3, 3, 3, 6] and h["win_hi"][s1].tolist() == [3, 3, 3, 3, 3, 3, 6, 10]
    assert np.isnan(h["row"][1:6]).all() and h["row"][0] == 6.0 and h["row"][7] == 34.5
    for L in (1, 2):
        ref = stk.handover(cells2, lab, ang, nx, 1.0)[L - 1]
        c, rg = stk.stations(ref[2], 4.0, 4.0)
        sl_ = slice(h["seg_win_start"][L - 1], h["seg_win_start"][L])
        k0 = h["seg_start"][L - 1]
        assert np.array_equal(h["t"][sl_], c) and [(a - k0, b - k0) for a, b in zip(h["win_lo"][sl_], h["win_hi"][sl_])] == rg
        assert np.array_equal(h["cells"][k0:h["seg_start"][L]], cells2[ref[1]])


def test_every_cell_lies_in_a_window():
    rng = np.random.default_rng(7)
    nx = 200
    for trial in range(200):
        de = float(rng.choice([0.5, 1.0, 2.0, 3.7]))
        window = de * float(rng.uniform(1.0, 40.0))
        step = float(rng.uniform(de, window))
        if trial % 10 == 0:
            step = window
        if trial % 10 == 1:
            step = de
        K = int(rng.integers(1, 120))
        cells = rng.integers(0, 150, K) * nx + rng.integers(0, nx, K)
        lab = rng.integers(1, 4, K)
        ang = rng.uniform(-np.pi / 2, np.pi / 2, K)
        h = handover((150, nx), de, cells, lab, ang, window, step)
        seen = np.zeros(K, dtype=int)
        for lo, hi in zip(h["win_lo"], h["win_hi"]):
            seen[lo:hi] += 1
        assert (seen >= 1).all(), (trial, de, window, step)
        S = len(h["seg_label"])
        for s in range(S):
            g0, g1 = h["seg_win_start"][s], h["seg_win_start"][s + 1]
            assert g1 > g0 and (h["win_lo"][g0:g1] >= h["seg_start"][s]).all() and (h["win_hi"][g0:g1] <= h["seg_start"][s + 1]).all()
            assert (np.diff(h["win_lo"][g0:g1]) >= 0).all() and (np.diff(h["win_hi"][g0:g1]) >= 0).all()
            assert np.allclose(np.diff(h["t"][g0:g1]), step)


def test_a_one_cell_segment():
    h = handover((40, 50), 2.0, [3 * 50 + 9, 700], [6, 2], [0.3, 1.0], 8.0)
    assert h["seg_label"].tolist() == [2, 6] and h["seg_win_start"].tolist() == [0, 1, 2]
    assert h["win_lo"].tolist() == [0, 1] and h["win_hi"].tolist() == [1, 2]
    # the station sits at its cell
    assert h["t"][1] == 2.0 * (3.0 * math.cos(0.3) + 9.0 * math.sin(0.3)) and h["row"].tolist() == [14.0, 3.0]
    assert h["col"].tolist() == [0.0, 9.0]
    # the strike is axial: an orientation and its opposite are one strike, folded into (-pi/2, pi/2]
    g = handover((40, 50), 2.0, [3 * 50 + 9, 700], [6, 2], [0.3 + np.pi, 1.0 - np.pi], 8.0)
    assert np.allclose(g["t"], h["t"], rtol=1e-12, atol=0)


# ---- every argument error is a ValueError before the library is loaded ---------------------------------------------------------
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
    ok = dict(data=g, cells=[3, 77], labels=[1, 1], angle=0.1, half_length=20.0, window=8.0)      # h = 10
    bad = [
        (dict(window=None), "window missing"),
        (dict(window=1.9), "window below the cell size"),
        (dict(window=np.nan), "window NaN"),
        (dict(window=np.inf), "window inf"),
        (dict(window="long"), "window not a number"),
        (dict(window=True), "window a bool"),
        (dict(step=1.9), "step below the cell size"),
        (dict(step=8.1), "step above the window"),
        (dict(step=np.nan), "step NaN"),
        (dict(step=np.inf), "step inf"),
        (dict(step="short"), "step not a number"),
        (dict(window=3.0), "window / 2 below the cell size and no step"),
        (dict(delta=-1.0), "delta < 0"),
        (dict(min_profiles=0), "min_profiles < 1"),
        (dict(min_samples=1), "min_samples < 2"),
        (dict(min_samples=11), "min_samples > h"),
        (dict(max_shift=-1.0), "max_shift < 0"),
        (dict(max_shift=14.0), "7 cells, more than h - min_samples = 6"),
        (dict(half_length=2.0), "h < 2"),
        (dict(swath=-1.0), "swath < 0"),
        (dict(ages=[3.0, 2.0]), "ages not increasing"),
        (dict(ages=[]), "no age"),
        (dict(cells=[3, 2000]), "a cell outside the grid"),
        (dict(labels=[1, 1, 1]), "labels of another length"),
        (dict(labels=[1.0, 1.0]), "labels not integers"),
        (dict(angle=[0.1, np.nan]), "angle NaN"),
        (dict(data=np.zeros((40, 50))), "data not a DEMGrid"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError):
            sl.fit_along_strike(**dict(ok, **kw))
            pytest.fail(what)
    with pytest.raises(ValueError):
        sl.fit_along_strike(g, [3, 77], [1, 1], 0.1, 20.0)                 # window has no default
    # what is valid gets as far as the device
    for kw in (dict(), dict(step=2.0), dict(step=8.0), dict(window=2.0, step=2.0), dict(window=3.0, step=2.5),
               dict(max_shift=13.9), dict(max_shift=0), dict(return_curve=True, min_profiles=2, delta=0.0)):
        with pytest.raises(AssertionError, match="the library was asked for"):
            sl.fit_along_strike(**dict(ok, **kw))


def test_matcher_route_validates():
    import scarplet_amd as sl
    from scarplet_amd import traces

    class Held(object):
        whole, ny, nx, de = True, 40, 50, 2.0
    tr = traces.Traces(np.zeros((40, 50), dtype=bool), np.zeros((40, 50), dtype=np.int32),
                       traces._table(np.zeros(0, dtype=_lib.SEGMENT_DTYPE)))
    for kw in (dict(window=1.0), dict(window=8.0, step=9.0), dict(window=8.0, step=1.0), dict(window=8.0, strike="both"),
               dict(window=8.0, min_profiles=0)):
        with pytest.raises(ValueError):
            sl.Matcher.fit_along_strike(Held(), tr, 20.0, strike=kw.pop("strike", "segment"), **kw)
    with pytest.raises(ValueError):
        sl.Matcher.fit_along_strike(Held(), "traces", 20.0, 8.0)
    part = Held()
    part.whole = False
    with pytest.raises(ValueError):
        sl.Matcher.fit_along_strike(part, tr, 20.0, 8.0)


def test_table_fields():
    assert strike.FIT_DTYPE.names == ("label", "station", "n_cells", "n_profiles", "n", "dof", "kt_index", "lo_index",
                                      "hi_index", "status", "kt", "kt_lo", "kt_hi", "a", "sse", "rmse", "height", "t", "row",
                                      "col")
    assert all(strike.FIT_DTYPE.fields[f][0] == np.float64 for f in ("height", "t", "row", "col"))
    import scarplet_amd as sl
    assert sl.fit_along_strike is strike.fit_along_strike and hasattr(sl.Matcher, "fit_along_strike")


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_strike_struct_layout_matches_c(tmp_path):
    S, dt = _lib.sc_strike_fit, _lib.STRIKE_FIT_DTYPE
    names = [f for f, _ in S._fields_]
    body = '  printf("%zu\\n", sizeof(sc_strike_fit));\n'
    body += "".join('  printf("%%zu\\n", offsetof(sc_strike_fit, %s));\n' % f for f in names)
    prog = tmp_path / "strike.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarplet_hip.h"\nint main(void) {\n' + body
                    + '  printf("%d %d\\n", SC_K_COUNT, SC_ABI_VERSION);\n  return 0;\n}\n')
    exe = tmp_path / "strike"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert vals == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in names] + [11, 10]
    assert ctypes.sizeof(S) == 88 and dt.itemsize == 88 and dt.names == tuple(names)
    assert [dt.fields[f][1] for f in names] == [getattr(S, f).offset for f in names]
    assert names == ["label", "station", "n_cells", "n_profiles", "n", "dof", "kt_index", "lo_index", "hi_index", "status",
                     "kt", "kt_lo", "kt_hi", "a", "sse", "rmse"]
    assert len(_lib.K_NAMES) == 11 and _lib.ABI_VERSION == 10


STRIKE_CALLS = ("sc_fit_strike", "sc_fit_strike_dem")


def test_header_declares_the_calls_and_keeps_the_abi():
    txt = open(os.path.join(ROOT, "include", "scarplet_hip.h")).read()
    assert "#define SC_ABI_VERSION 10\n" in txt
    assert re.search(r"#define\s+SC_K_COUNT\s+11\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for n in STRIKE_CALLS:
        assert re.search(r"\bint %s\s*\(" % n, code), n
        assert len(_lib.SIGNATURES[n][1]) == 23 + (3 if n.endswith("_dem") else 0)


def test_library_exports_the_calls():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in STRIKE_CALLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert _lib.load().sc_abi_version() == 10


def test_build_id_covers_the_new_source():
    mk = open(os.path.join(ROOT, "scarplet_amd", "csrc", "Makefile")).read()
    src = re.search(r"^SRC\s*=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "sc_strike.hip" in src and re.search(r"^ID_SRC\s*=\s*\$\(SRC\) \$\(HDR\)$", mk, flags=re.M)


def test_strike_kernels_fit_their_budget():
    from test_isa_budget import kernel_table
    t = kernel_table("sc_strike.hip")
    for k in ("k_st_spp", "k_st_fit"):
        assert k in t, sorted(t)
        assert t[k]["scratch"] == 0, (k, t[k])
        assert t[k]["vgpr"] + t[k]["agpr"] <= 128, (k, t[k])               # four waves per SIMD
    # stage one stays where it was, with its budget
    s = kernel_table("sc_segment.hip")
    for k in ("k_sg_partial<true>", "k_sg_partial<false>", "k_sg_shift<true>", "k_sg_shift<false>", "k_sg_rank"):
        assert k in s and s[k]["scratch"] == 0 and s[k]["vgpr"] + s[k]["agpr"] <= 128, (k, s.get(k))


# ---- the restatement on the noisy case of docs/segments.md ----------------------------------------------------------------
def test_restatement_on_the_noisy_case():
    """h = 100, w = 2, the default ages, window 60 and step 30: eleven stations of 11 to 20 profiles each.  The surface
    was made with kt = 10, index 10 of the grid.  A single profile finds it 18 times in 100 and the pooled hundred
    always (docs/segments.md); windows of about twenty are between the two: every station within one grid step (0.1
    decades) of the true index, most of them on it, and every amplitude within 2 % of 1."""
    z, cells, theta = sr.noisy_case()
    rows = stk.fit_along_strike(z, 1.0, cells, np.ones(100, dtype=int), theta, 100, 2, AGES, 60.0, 30.0, min_samples=15)
    idx = [r["kt_index"] for r in rows]
    print(idx, [round(r["a"], 4) for r in rows])
    assert len(rows) == 11 and [r["station"] for r in rows] == list(range(11))
    assert [r["n_cells"] for r in rows] == [11, 20, 19, 19, 20, 20, 20, 19, 19, 20, 11]
    assert all(r["n_profiles"] == r["n_cells"] and r["status"] == 0 for r in rows)
    assert all(abs(i - 10) <= 1 for i in idx) and sum(i == 10 for i in idx) >= 6
    assert all(abs(r["a"] - 1.0) <= 0.02 for r in rows)
    assert all(r["spp"] <= 8.7 * r["curve"].min() and r["cond"] <= 1e3 for r in rows)
    # the stations are centred on the segment, 30 apart
    t = np.array([r["t"] for r in rows])
    tc = np.sort((cells // 600) * np.cos(theta) + (cells % 600) * np.sin(theta))
    assert np.allclose(np.diff(t), 30.0) and abs((t[0] + t[-1]) / 2 - (tc[0] + tc[-1]) / 2) < 1e-9
