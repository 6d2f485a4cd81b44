"""Traces of a result, on the CPU: the numpy reference (tests/trace_reference.py) on hand-built planes with known
answers, argument validation of sl.extract_traces before any device call, the sc_segment layout, and the kernels'
scratch budget."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import trace_reference as tr
from scarplet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = tr.PI


def planes(snr, ang):
    snr = np.asarray(snr, dtype=np.float64)
    ang = np.broadcast_to(np.asarray(ang, dtype=np.float64), snr.shape).copy()
    amp = np.arange(snr.size, dtype=np.float64).reshape(snr.shape) * 0.5 - 3.0
    age = np.full(snr.shape, 10.0)
    return np.stack([amp, age, ang, snr])


def ridge(n, dist):
    """n x n snr falling off with the distance ``dist(r, c)`` from a line (peak 10)."""
    r, c = np.mgrid[0:n, 0:n]
    return 10.0 - np.abs(dist(r, c)).astype(np.float64)


# ---- the reference on hand-built planes ------------------------------------------------------------------------
@pytest.mark.parametrize("a, dist, want", [
    (0.0, lambda r, c: c - 5, lambda r, c: c == 5),                 # sector 0: profile along the columns
    (PI / 2, lambda r, c: r - 4, lambda r, c: r == 4),              # sector 2: along the rows
    (PI / 4, lambda r, c: r - c, lambda r, c: r == c),              # sector 1: step (+1, -1), line r = c
    (-PI / 4, lambda r, c: r + c - 9, lambda r, c: r + c == 9),     # sector 3: step (+1, +1), line r + c = 9
])
def test_line_in_each_sector(a, dist, want):
    # only the line clears snr_low: a step along the line instead of across it would keep one cell of the plateau
    n = 10
    t, labels, tab = tr.trace(planes(ridge(n, dist), a), 9.5)
    r, c = np.mgrid[0:n, 0:n]
    assert np.array_equal(t, want(r, c))
    assert labels.max() == 1 and np.array_equal(labels > 0, t)
    assert tab["n_cells"][0] == t.sum() and tab["first"][0] == np.flatnonzero(t.ravel())[0]


def test_sectors_on_boundaries_and_beyond():
    a = np.array([0.0, PI / 8, -PI / 8, PI / 4, -PI / 4, PI / 2, -PI / 2, 3 * PI / 4, -3 * PI / 4, PI, -PI,
                  5 * PI / 8, 9 * PI / 8, 4.5 * PI, -5 * PI])
    s = tr.sectors(a)
    # +pi/8 rounds up into sector 1, -pi/8 into sector 0 (floor(x + 0.5)); the sectors repeat every pi
    assert list(s[:11]) == [0, 1, 0, 1, 3, 2, 2, 3, 1, 0, 0]
    q = np.floor((a / PI) * 4.0 + 0.5)
    assert np.array_equal(s, (q % 4).astype(int))
    rng = np.random.default_rng(1)
    x = rng.uniform(-3, 3, 1000)
    assert np.array_equal(tr.sectors(x), tr.sectors(x + PI)) or \
        (tr.sectors(x) != tr.sectors(x + PI)).sum() <= 2          # (x + pi rounds: boundary cells only)


def test_plateau_keeps_exactly_one_cell():
    snr = np.array([[0.5, 1.0, 5.0, 5.0, 1.0, 0.5]])
    t, _, _ = tr.trace(planes(snr, 0.0), 0.7)
    assert list(np.flatnonzero(t[0])) == [2]


def test_nan_neighbour_and_nan_cell():
    snr = np.array([[np.nan, 3.0, 1.0, 2.0, np.inf]])
    t, _, _ = tr.trace(planes(snr, 0.0), 0.5)
    # cell 1: left is NaN (-inf), right 1 -> kept; cell 3: right is inf, not finite (-inf) -> kept; NaN and inf
    # cells are not valid
    assert list(np.flatnonzero(t[0])) == [1, 3]
    ang = np.zeros((1, 5))
    ang[0, 1] = np.nan
    t, _, _ = tr.trace(planes(snr, ang), 0.5)
    assert not t[0, 1]


def test_invalid_cells():
    snr = np.array([[2.0, 0.0, 2.0, -1.0, 2.0, 2.0]])
    ang = np.array([[0.0, 0.0, 2e6, 0.0, np.inf, 0.0]])
    t, _, _ = tr.trace(planes(snr, ang), 0.5)
    # cells 1 - 4 are not valid; cell 5 is, but its left neighbour's finite snr still counts (2 > 2 fails)
    assert list(np.flatnonzero(t[0])) == [0]


def test_edge_and_corner_cells():
    t, labels, tab = tr.trace(planes(np.array([[5.0]]), 0.3), 1.0)
    assert t.all() and labels[0, 0] == 1 and tab["n_cells"][0] == 1
    snr = np.full((3, 3), 1.0)
    snr[0, 0] = snr[2, 2] = 4.0
    t, _, _ = tr.trace(planes(snr, -PI / 4), 0.5)           # step (+1, +1): the corners have one neighbour each
    assert t[0, 0] and t[2, 2] and not t[1, 1]


def sparse(ny, nx, cells, snr=2.0):
    """snr at the given cells, 0 (not valid) elsewhere; angle 0 - every such cell not next to another in its row is thin"""
    s = np.zeros((ny, nx))
    for (r, c) in cells:
        s[r, c] = snr if np.isscalar(snr) else snr[(r, c)]
    return planes(s, 0.0)


def test_diagonal_runs_are_one_segment():
    p = sparse(4, 6, [(0, 0), (1, 1), (2, 2), (3, 4)])
    t, labels, tab = tr.trace(p, 1.0)
    assert t.sum() == 4
    assert list(tab["n_cells"]) == [3, 1]
    assert labels[2, 2] == 1 and labels[3, 4] == 2
    p = sparse(3, 4, [(0, 3), (1, 2), (2, 1)])               # the other diagonal
    assert list(tr.trace(p, 1.0)[2]["n_cells"]) == [3]


def test_hysteresis_drops_weak_only_components():
    snr = {(0, 0): 5.0, (1, 1): 2.0, (0, 4): 2.0, (1, 5): 2.0}
    p = sparse(3, 7, list(snr), snr)
    t, labels, tab = tr.trace(p, 1.0, 4.0)
    assert t.sum() == 4
    assert list(tab["n_cells"]) == [2] and list(tab["n_strong"]) == [1]
    assert labels[1, 1] == 1 and labels[0, 4] == 0 and labels[1, 5] == 0


def test_min_cells():
    p = sparse(5, 8, [(0, 0), (1, 1), (2, 2), (0, 6), (4, 4)])
    assert list(tr.trace(p, 1.0, min_cells=2)[2]["n_cells"]) == [3]
    assert list(tr.trace(p, 1.0, min_cells=1)[2]["n_cells"]) == [3, 1, 1]
    assert len(tr.trace(p, 1.0, min_cells=4)[2]["n_cells"]) == 0


def test_label_order_is_smallest_index():
    # segment A starts at (0, 5); B's cells lie further left but start one row lower
    p = sparse(4, 8, [(1, 0), (2, 1), (3, 2), (0, 5), (1, 6)])
    t, labels, tab = tr.trace(p, 1.0)
    assert list(tab["first"]) == [5, 8]
    assert labels[0, 5] == 1 and labels[1, 0] == 2
    assert list(tab["row_min"]) == [0, 1] and list(tab["row_max"]) == [1, 3]
    assert list(tab["col_min"]) == [5, 0] and list(tab["col_max"]) == [6, 2]


def test_table_peak_and_sums():
    snr = {(0, 0): 3.0, (1, 1): 7.0, (2, 2): 7.0, (3, 3): 1.5}
    p = sparse(4, 5, list(snr), snr)
    p[2] = 0.3
    t, labels, tab = tr.trace(p, 1.0, 5.0)
    assert list(tab["peak"]) == [6]                           # (1, 1): the tie with (2, 2) goes to the smaller index
    assert tab["snr_peak"][0] == 7.0 and tab["amp_peak"][0] == p[0].ravel()[6]
    assert tab["n_strong"][0] == 2
    idx = np.flatnonzero(labels.ravel())
    assert tab["sum_snr"][0] == p[3].ravel()[idx].sum()
    assert np.isclose(tab["sum_cos2a"][0], 4 * np.cos(0.6)) and np.isclose(tab["sum_sin2a"][0], 4 * np.sin(0.6))


# ---- sl.extract_traces validates before any device call --------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    import scarplet_amd.core as core

    def refuse(device):
        raise AssertionError("a device was asked for")
    monkeypatch.setattr(core, "_context", refuse)


def test_extract_traces_validates_without_a_device(no_device):
    import scarplet_amd as sl
    ok = planes(np.ones((3, 4)), 0.0)
    bad = [
        (dict(results=np.ones((3, 3, 4))), "shape"),
        (dict(results=np.ones((4, 5))), "ndim"),
        (dict(results=(ok[0], ok[1], ok[2])), "three planes"),
        (dict(results=(ok[0], ok[1], ok[2], ok[3][:2])), "planes of two shapes"),
        (dict(results=ok, snr_low=np.nan), "snr_low NaN"),
        (dict(results=ok, snr_low=np.inf), "snr_low inf"),
        (dict(results=ok, snr_low=0.0), "snr_low 0"),
        (dict(results=ok, snr_low=-1.0), "snr_low < 0"),
        (dict(results=ok, snr_low=2.0, snr_high=1.0), "snr_high < snr_low"),
        (dict(results=ok, snr_low=2.0, snr_high=np.nan), "snr_high NaN"),
        (dict(results=ok, min_cells=0), "min_cells 0"),
        (dict(results=ok, min_cells=1.5), "min_cells not an integer"),
        (dict(results=np.broadcast_to(np.float64(1.0), (4, 46341, 46341))), "more than 2^31 - 1 cells"),
        (dict(results=tuple(np.broadcast_to(np.float64(1.0), (65536, 32768)) for _ in range(4))), "tuple, too many cells"),
    ]
    for kw, what in bad:
        kw.setdefault("snr_low", 1.0)
        with pytest.raises(ValueError):
            sl.extract_traces(**kw)
            pytest.fail(what)


def test_extract_traces_is_exported():
    import scarplet_amd as sl
    assert callable(sl.extract_traces)
    assert sl.Traces._fields == ("thin", "labels", "segments")


# ---- the C ABI ---------------------------------------------------------------------------------------------------
def test_segment_layout_matches_c(tmp_path):
    names = [f for f, _ in _lib.sc_segment._fields_]
    prog = tmp_path / "seg.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scarplet_hip.h"\nint main(void) {\n'
                    '  printf("%zu\\n", sizeof(sc_segment));\n'
                    + "".join('  printf("%%zu\\n", offsetof(sc_segment, %s));\n' % f for f in names)
                    + "  return 0;\n}\n")
    exe = tmp_path / "seg"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    S = _lib.sc_segment
    assert vals == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in names]
    assert _lib.SEGMENT_DTYPE.itemsize == ctypes.sizeof(S)
    assert "SC_K_TRACE" in open(os.path.join(ROOT, "include", "scarplet_hip.h")).read()
    assert _lib.K_NAMES[_lib.K_TRACE] == "k_trace"


def test_library_exports_the_trace_calls():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("sc_trace_planes", "sc_trace_result", "sc_trace_segments"):
        assert hasattr(lib, n)
    assert _lib.load().sc_kernel_name(_lib.K_TRACE) == b"k_trace"


def test_trace_kernels_have_no_scratch():
    from test_isa_budget import kernel_table
    t = kernel_table("sc_trace.hip")
    for k in ("k_tr_thin", "k_tr_local", "k_tr_merge", "k_tr_flatten", "k_tr_rs_hist", "k_tr_rs_scatter",
              "k_tr_reduce", "k_tr_scan_top"):
        assert k in t, sorted(t)
    assert len(t) >= 14
    for name, r in t.items():
        assert r["scratch"] == 0, (name, r)
