"""The initial slope of sl.fit_segments on the MI355X (sc_fit_segments_ramp; docs/segments.md, "The initial slope") against
the numpy restatement (tests/segment_ramp_reference.py).

Tolerances are those of tests/test_gpu_segments.py and tests/test_gpu_ramp.py and stand on the same ground: every compared
(age, half-width) has a column-scaled full design matrix of condition number <= 1e3 and the float64 restatement agrees
with its longdouble twin within 1e-11 there (asserted on the CPU, tests/test_segment_ramp_host.py; the age grids of the
cases are cut to it, segment_ramp_reference.NA), so the pooled sse, sse* and every profile's share agree within 1e-9
relative and a, b h de, c0 within 1e-9 of the largest range of a profile.  An m_i or an index that differs from the
restatement's must have been decided within 1e-9 relative by the restatement's own key; segments with such a decision may
be at most 1 % of a case.  The anchors are byte comparisons.
"""
import numpy as np
import pytest

import profile_reference as pr
import ramp_reference as rr
import segment_ramp_reference as sx
import scarplet_amd as sl
from scarplet_amd import _lib, _plan, synthetic

pytestmark = pytest.mark.gpu

MODES = [sx.FREE, sx.SLOPE]


def grid(z, de):
    return sl.DEMGrid.from_array(z, float(de))


def run(case, mode=sx.FREE, M="case", labels=None, **kw):
    h, w, de = case["h"], case["w"], case["de"]
    M = case["M"] if M == "case" else M
    return sl.fit_segments(grid(case["z"], de), case["cells"], case["labels"] if labels is None else labels, case["angle"],
                           h * de, w * de, ages=case["ages"], delta=case["delta"], min_samples=case["min_samples"],
                           min_profiles=case["min_profiles"], max_width=None if M is None else M * de,
                           initial_slope=case["slope"] if mode == sx.SLOPE else None, **kw)


def run_profiles(case, mode, **kw):
    h, w, de = case["h"], case["w"], case["de"]
    return sl.fit_profiles(grid(case["z"], de), case["cells"], case["angle"], h * de, w * de, ages=case["ages"],
                           delta=case["delta"], min_samples=case["min_samples"], max_width=case["M"] * de,
                           initial_slope=case["slope"] if mode == sx.SLOPE else None, **kw)


CASES = None


def cases():
    global CASES
    if CASES is None:
        CASES = sx.gpu_cases()
    return CASES


def case_of(name):
    return cases()[sx.NAMES.index(name)]


def by_input_position(case, cell_table):
    kept = np.flatnonzero(case["labels"] > 0)
    assert len(cell_table) == len(kept)
    assert np.array_equal(cell_table["cell"], case["cells"][kept]) and np.array_equal(cell_table["label"], case["labels"][kept])
    full = np.zeros(len(case["cells"]), dtype=cell_table.dtype)
    full[kept] = cell_table
    return full


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sx.NAMES)
def test_against_the_restatement(name, mode):
    case = case_of(name)
    table, cells, curve, widths = run(case, mode, return_cells=True, return_curve=True, return_width=True)
    ref = sx.restate(case, mode)
    S, A, M = len(ref), len(case["ages"]), case["M"]
    assert table.dtype.names[-4:] == ("width_index", "width", "initial_slope", "height") and len(table) == S
    assert cells.dtype.names[-1] == "label" and "shift" not in cells.dtype.names
    assert curve.shape == (S, A) and widths.shape == (S, A) and widths.dtype == np.int8
    st = sx.compare_segments(ref, table, by_input_position(case, cells), curve, widths, case["h"], case["de"], M, mode,
                             case["slope"], case["delta"])
    print("%s, mode %d: %s" % (name, mode, st))
    free = 1 if mode == sx.FREE and M > 0 else 0
    assert np.array_equal(table["dof"], table["n"] - 2 * table["n_profiles"] - 1 - free)
    fit = table["status"] != 1
    assert np.array_equal(table["kt"][fit], case["ages"][table["kt_index"][fit]])
    assert np.array_equal(table["kt_lo"][fit], case["ages"][table["lo_index"][fit]])
    assert np.array_equal(table["kt_hi"][fit], case["ages"][table["hi_index"][fit]])
    assert np.array_equal(curve[fit, table["kt_index"][fit]], table["sse"][fit])
    if name in ("h100 w0 M8", "h30 w5 M4"):
        assert S == 8 and st["fitted"] == 8 and np.any(np.diff(case["labels"]) < 0)
    if name == "sizes 1 2 64 65 130":
        assert sorted(table["n_profiles"]) == [1, 2, 64, 65, 130] and st["fitted"] == 5
    if name == "repeated cells":
        assert st["fitted"] == 2 and list(table["n_profiles"]) == [5, 15]
    if name in ("no cell", "labels <= 0 only"):
        assert len(table) == 0 and len(cells) == 0 and curve.shape == (0, A)
    if name == "unusable segment":
        assert list(table["label"]) == [4, 6] and list(table["n_profiles"]) == [0, 2] and list(table["status"] & 1) == [1, 0]
    if name == "borders":
        assert (cells["used"] == 0).sum() >= 5 and st["fitted"] >= 3
    if name == "NaN cells":
        assert (cells["n"][cells["used"] == 1] < 2 * case["h"] + 1).sum() >= 5
    if name == "min_profiles 5":
        assert sorted(table["status"] & 1) == [0, 0, 0, 1, 1, 1] and (table["n_profiles"][table["status"] == 1] > 0).all()
    if name == "dof < 1 with the width free":
        assert list(table["n_profiles"]) == [1, 3] and list(table["n"]) == [4, 21]
        assert list(table["status"] & 1) == ([1, 0] if mode == sx.FREE else [0, 0])
        assert list(table["dof"]) == ([0, 13] if mode == sx.FREE else [1, 14])
    # a second run, and the runs without the optional outputs: the same bytes
    t2, c2, v2, w2 = run(case, mode, return_cells=True, return_curve=True, return_width=True)
    assert t2.tobytes() == table.tobytes() and c2.tobytes() == cells.tobytes() and v2.tobytes() == curve.tobytes()
    assert w2.tobytes() == widths.tobytes()
    assert run(case, mode).tobytes() == table.tobytes()
    t3, w3 = run(case, mode, return_width=True)
    assert t3.tobytes() == table.tobytes() and w3.tobytes() == widths.tobytes()


# ---- the anchors, as bytes ---------------------------------------------------------------------------------------------------
def same_bytes(a, b, fields):
    for f in fields:
        assert a[f].tobytes() == b[f].tobytes(), f


@pytest.mark.parametrize("name", ["h100 w0 M8", "h30 w5 M4", "sizes 1 2 64 65 130", "64 ages M1", "borders", "unusable segment",
                                  "NaN cells", "min_profiles 5"])
def test_a_range_of_zero_is_the_plain_call(name):
    case = case_of(name)
    base, bcells, bcurve = run(case, M=None, return_cells=True, return_curve=True)
    zero, zcells, zcurve, zw = run(case, M=0, return_cells=True, return_curve=True, return_width=True)
    assert "width" not in base.dtype.names and len(base) == len(zero)
    same_bytes(zero, base, base.dtype.names)
    assert zcells.dtype == bcells.dtype and zcells.tobytes() == bcells.tobytes() and zcurve.tobytes() == bcurve.tobytes()
    assert not zw.any() and not zero["width_index"].any()
    fit = zero["status"] != 1
    assert fit.sum() >= 1 and np.all(zero["width"][fit] == 0.0) and np.isnan(zero["width"][~fit]).all()
    assert np.array_equal(zero["initial_slope"][fit], np.copysign(np.inf, zero["a"][fit]))
    assert np.isnan(zero["initial_slope"][~fit]).all()


@pytest.mark.parametrize("mode", MODES)
def test_one_profile_segments_are_the_single_fit_byte_for_byte(mode):
    by = {c["name"]: c for c in rr.gpu_cases()}
    for name in ("h100 w0 M8", "h30 w5 M4", "borders and corners", "NaN cells", "M = h - min_samples", "64 ages M1"):
        case = dict(by[name], min_profiles=1)
        K = len(case["cells"])
        lab = np.random.default_rng(3).permutation(K) + 1                  # one segment per cell, in shuffled order
        seg, ct, cv, wp = run(case, mode, labels=lab, return_cells=True, return_curve=True, return_width=True)
        one, ocv, owp = run_profiles(case, mode, return_curve=True, return_width=True)
        fit = one["status"] != 1
        assert fit.sum() >= K // 4
        for f in ("b", "c0", "sse", "cell", "n"):
            assert ct[f].tobytes() == one[f].tobytes(), (name, f)
        order = np.argsort(lab)                                            # in label order
        one, ocv, owp = one[order], ocv[order], owp[order]
        for f in ("kt_index", "lo_index", "hi_index", "status", "a", "sse", "rmse", "kt", "kt_lo", "kt_hi", "height",
                  "width_index", "width", "initial_slope"):
            assert seg[f].tobytes() == one[f].tobytes(), (name, f)
        assert cv.tobytes() == ocv.tobytes() and wp.tobytes() == owp.tobytes()
        fit = one["status"] != 1
        free = 1 if mode == sx.FREE else 0
        assert np.array_equal(seg["dof"][fit], one["n"][fit] - 3 - free) and (seg["n_cells"] == 1).all()


@pytest.mark.parametrize("mode", MODES)
def test_reordering_whole_segments_gives_the_same_rows(mode):
    case = case_of("sizes 1 2 64 65 130")
    table, cells, curve, widths = run(case, mode, return_cells=True, return_curve=True, return_width=True)
    # the segments in another order of arrival, the order inside a label kept
    pos = np.concatenate([np.flatnonzero(case["labels"] == l) for l in (9, 7, 1, 5, 2)])
    moved = dict(case, cells=case["cells"][pos], labels=case["labels"][pos], angle=case["angle"][pos])
    t2, c2, v2, w2 = run(moved, mode, return_cells=True, return_curve=True, return_width=True)
    assert t2.tobytes() == table.tobytes() and v2.tobytes() == curve.tobytes() and w2.tobytes() == widths.tobytes()
    assert c2.tobytes() == cells[pos].tobytes()


def test_matcher_route_gives_the_same_bytes():
    g = synthetic.synthetic_scarp(768, theta=0.6)
    m = sl.Matcher(g)
    m.search(sl.Scarp, 100., _plan.age_grid()[::5], _plan.angle_grid())
    res = np.array(m.result_array())
    lo, hi = np.percentile(res[3][res[3] > 0], [60, 90])
    tr = m.extract_traces(lo, hi, 4)
    cells = np.flatnonzero(tr.labels.ravel() > 0)
    assert len(cells) > 50 and len(tr.segments) > 1
    for kw in (dict(max_width=4.0), dict(max_width=4.0, initial_slope=0.3)):
        kw.update(return_cells=True, return_curve=True, return_width=True)
        a = m.fit_segments(tr, 60., 3., **kw)
        b = sl.fit_segments(g, cells, tr.labels, res[2], 60., 3., **kw)
        assert len(a) == 4 and all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and (a[0]["status"] != 1).sum() >= 1
        assert a[0].dtype.names[-4:] == ("width_index", "width", "initial_slope", "height")
    # the search's record is what it was
    assert np.array_equal(np.array(m.result_array()), res, equal_nan=True)


# ---- what it is for --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", [0.02, 0.05])
def test_the_recovery_case_on_the_device(noise):
    """docs/segments.md: a scarp that began as a ramp of six cells dates two grid steps too old under the plain joint fit;
    with the shared width, free or from the given slope, the joint fit returns the true index and the planted width, and
    its rows are the restatement's (the longdouble twin; tests/test_segment_ramp_host.py holds the lstsq restatement to
    the same figures)."""
    R = rr.REC
    z, cells, theta, ages = rr.recovery_case(noise)
    g = grid(z, 1.0)
    lab = np.ones(len(cells), dtype=int)
    plain = sl.fit_segments(g, cells, lab, theta, float(R["h"]), float(R["w"]))[0]
    assert plain["kt_index"] == 12
    for mode in MODES:
        row = sl.fit_segments(g, cells, lab, theta, float(R["h"]), float(R["w"]), max_width=float(R["M"]),
                              initial_slope=R["slope"] if mode == sx.SLOPE else None)[0]
        ref = sx.recovery_rows(noise, mode)[0]
        print("noise %g, mode %d: index %d [%d, %d], m = %d, a %.5f, slope %.5f, status %d"
              % (noise, mode, row["kt_index"], row["lo_index"], row["hi_index"], row["width_index"], row["a"],
                 row["initial_slope"], row["status"]))
        for f in ("n_profiles", "n", "dof", "kt_index", "lo_index", "hi_index", "status", "width_index"):
            assert int(row[f]) == ref[f], (mode, f, row[f], ref[f])
        assert (row["kt_index"], row["width_index"], row["lo_index"], row["hi_index"]) == (R["index"], R["L"], R["index"], R["index"])
        assert abs(row["sse"] - float(ref["sse"])) <= sx.RTOL * float(ref["sse"]) and abs(row["a"] - float(ref["a"])) <= sx.RTOL * ref["ptp"]
        assert row["n_profiles"] == 100 and row["status"] == 0


def test_status_8_says_the_range_ended_before_the_fit_did():
    """A planted half-width of 6 cells on an age grid that ends at the true age: with max_width = 3 the best width is the end
    of the range and the bit is set; with max_width = 8 it is not."""
    R = rr.REC
    z, cells, theta, ages = rr.recovery_case()
    g = grid(z, 1.0)
    lab = np.arange(len(cells)) // 50 + 1
    kw = dict(ages=ages[:R["index"] + 1])
    short = sl.fit_segments(g, cells, lab, theta, float(R["h"]), float(R["w"]), max_width=3.0, **kw)
    wide = sl.fit_segments(g, cells, lab, theta, float(R["h"]), float(R["w"]), max_width=8.0, **kw)
    assert len(short) == 2 and (short["width_index"] == 3).all() and (short["status"] & 8 == 8).all()
    assert (wide["width_index"] == R["L"]).all() and (wide["status"] & 8 == 0).all() and (wide["kt_index"] == R["index"]).all()


def test_library_refuses_what_the_header_says(gpu_ctx):
    ctx = _lib.Context(0)
    z = pr.synthetic_z(64)
    ages = np.array([1.0, 2.0])
    i64, i32 = (lambda v: np.array(v, dtype=np.int64)), (lambda v: np.array(v, dtype=np.int32))
    cells, sa, ca = i64([5 * 64 + 30, 6 * 64 + 30]), np.zeros(2), np.ones(2)

    def segs(M, h=10, ms=4, mode=_lib.RAMP_FREE, slope=0.0, start=(0, 1, 2), label=(1, 2), mp=1, dem=z):
        return ctx.fit_segments_ramp(cells, sa, ca, i64(start), i32(label), ages, h, 1, 1.0, 1.0, ms, mp, M, mode=mode,
                                     slope=slope, z=dem)
    assert (segs(6)[0]["status"] & 1 == 0).all()                           # M = h - min_samples is the last one taken
    assert (segs(6, mode=_lib.RAMP_SLOPE, slope=0.3)[0]["status"] & 1 == 0).all()
    for kw in (dict(M=-1), dict(M=7), dict(M=5, ms=6), dict(M=2, mode=2), dict(M=0, mode=_lib.RAMP_SLOPE, slope=0.3),
               dict(M=2, mode=_lib.RAMP_SLOPE, slope=0.0), dict(M=2, mode=_lib.RAMP_SLOPE, slope=np.nan),
               dict(M=2, mode=_lib.RAMP_SLOPE, slope=np.inf), dict(M=2, start=(0, 2, 1)), dict(M=2, label=(2, 1)),
               dict(M=2, label=(0, 1)), dict(M=2, mp=0)):
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-1\)"):
            segs(**kw)
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\)"):
        segs(65, h=100)
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-3\)"):
        segs(2, dem=None)                                                  # no DEM set
    # a segment above the park cap: 64 ages, h = 66 and M = 64 park 8 (133 + 4 64 65) bytes per cell, 32008 cells - where the
    # plain call's cap, 8 (133 + 4 64) bytes per cell, lies above a million
    cap = _lib.SEGMENT_MAX_PARK // (8 * (133 + 4 * 64 * 65))
    big = cap + 1
    assert cap == 32008 and _lib.SEGMENT_MAX_PARK // (8 * (133 + 4 * 64)) > 10 ** 6
    many, zeros, ones = np.full(big, 5 * 64 + 30, dtype=np.int64), np.zeros(big), np.ones(big)
    kt = 10 ** np.linspace(0, 2, 64)
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\).*a segment of 32009 cells, more than 32008"):
        ctx.fit_segments_ramp(many, zeros, ones, i64([0, big]), i32([1]), kt, 66, 0, 1.0, 1.0, 2, 1, 64, z=z)
    ctx.close()
