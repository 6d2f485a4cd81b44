"""The centre shift of sl.fit_profiles / sl.fit_segments on the MI355X (sc_fit_profiles_shift, sc_fit_segments_shift;
docs/profiles.md "The centre shift", docs/segments.md) against the numpy restatement (tests/shift_reference.py).

Tolerances are those of tests/test_gpu_profiles.py and stand on the same ground: every compared (age, shift) has a
column-scaled design matrix of condition number <= 1e3 (asserted on the restatement; the age grids of the cases are cut
to it, shift_reference.NA), so sse* and the sse of the chosen pair agree within 1e-9 relative and c0, b h de, a within 1e-9
of the profile's peak-to-peak range.  A shift d_i or an index that differs from the restatement's must have been decided
within 1e-9 relative by the restatement's own sse; cells with such a decision may be at most 1 % of a case.  The joint
restatement is run WITH the device's d_ci, each entry verified first, so a tie of stage one cannot cascade into the
segment's fit.  The anchors are byte comparisons.
"""
import numpy as np
import pytest

import profile_reference as pr
import segment_reference as sr
import shift_reference as sh
import scarplet_amd as sl
from scarplet_amd import _lib, _plan, synthetic

pytestmark = pytest.mark.gpu


def grid(z, de):
    return sl.DEMGrid.from_array(z, float(de))


def run_profiles(case, D="case", **kw):
    h, w, de = case["h"], case["w"], case["de"]
    D = case["D"] if D == "case" else D
    return sl.fit_profiles(grid(case["z"], de), case["cells"], case["angle"], h * de, w * de, ages=case["ages"],
                           delta=case["delta"], min_samples=case["min_samples"], max_shift=None if D is None else D * de, **kw)


def run_segments(case, D="case", labels=None, **kw):
    h, w, de = case["h"], case["w"], case["de"]
    D = case["D"] if D == "case" else D
    return sl.fit_segments(grid(case["z"], de), case["cells"], case["labels"] if labels is None else labels, case["angle"],
                           h * de, w * de, ages=case["ages"], delta=case["delta"], min_samples=case["min_samples"],
                           min_profiles=case.get("min_profiles", 1), max_shift=None if D is None else D * de, **kw)


def restate_profiles(case):
    return sh.fit_profiles(case["z"], case["de"], case["cells"], case["angle"], case["h"], case["w"], case["D"], case["ages"],
                           case["delta"], case["min_samples"])


PCASES = SCASES = None


def pcases():
    global PCASES
    if PCASES is None:
        PCASES = sh.profile_cases()
    return PCASES


def scases():
    global SCASES
    if SCASES is None:
        SCASES = sh.segment_cases()
    return SCASES


PNAMES = ["synthetic h100 w0 D8", "synthetic h100 w5 D1", "synthetic h30 w5 D4", "64 ages", "one age", "repeated cells",
          "D = h - min_samples", "no cell", "borders and corners", "NaN cells"]
SNAMES = ["segments h100 w0 D8", "segments h30 w5 D4", "sizes 1 2 64 65 300", "shuffled order", "unusable segment", "no cell",
          "table in global memory"]


def test_the_case_lists_are_the_ones_named_here():
    assert [c["name"] for c in pcases()] == PNAMES and [c["name"] for c in scases()] == SNAMES
    for c in pcases() + scases():
        assert 0 <= c["D"] <= min(_lib.PROFILE_MAX_SHIFT, c["h"] - c["min_samples"]) and len(c["cells"]) <= 500
    assert {(c["h"], c["w"], c["D"]) for c in pcases()[:3]} == {(100, 0, 8), (100, 5, 1), (30, 5, 4)}
    edge = pcases()[PNAMES.index("D = h - min_samples")]
    assert edge["D"] == edge["h"] - edge["min_samples"]


@pytest.mark.parametrize("name", PNAMES)
def test_profiles_against_the_restatement(name):
    case = pcases()[PNAMES.index(name)]
    table, curve, shifts = run_profiles(case, return_curve=True, return_shift=True)
    K, A = len(case["cells"]), len(case["ages"])
    assert table.dtype.names[-2:] == ("shift_index", "shift") and len(table) == K
    assert curve.shape == (K, A) and shifts.shape == (K, A) and shifts.dtype == np.int8
    nx = case["z"].shape[1]
    assert np.array_equal(table["cell"], case["cells"]) and np.array_equal(table["row"] * nx + table["col"], case["cells"])
    ref = restate_profiles(case)
    st = sh.compare_rows(ref, table, curve, shifts, case["h"], case["de"], case["D"], case["delta"])
    print("%s: %s" % (name, st))
    fit = table["status"] != 1
    assert np.array_equal(table["kt"][fit], case["ages"][table["kt_index"][fit]])
    assert np.array_equal(table["kt_lo"][fit], case["ages"][table["lo_index"][fit]])
    assert np.array_equal(table["kt_hi"][fit], case["ages"][table["hi_index"][fit]])
    assert np.array_equal(curve[fit, table["kt_index"][fit]], table["sse"][fit])
    assert np.abs(shifts).max(initial=0) <= case["D"]
    if name == "no cell":
        assert K == 0
    elif name in ("borders and corners", "NaN cells"):
        n = np.array([r["n"] for r in ref])
        assert (~fit).sum() > 0 or name == "NaN cells"
        # fitted with points missing (a property of the inputs: 26 and 9 such cells on the restatement)
        assert (fit & (n < 2 * case["h"] + 1)).sum() >= 5
    else:
        assert st["fitted"] == K
    if name == "repeated cells":
        for k in range(0, K, 3):
            assert table[k:k + 3].tobytes() == table[k:k + 1].tobytes() * 3
    # a second run and the runs without the optional outputs: the same bytes
    t2, c2, s2 = run_profiles(case, return_curve=True, return_shift=True)
    assert t2.tobytes() == table.tobytes() and c2.tobytes() == curve.tobytes() and s2.tobytes() == shifts.tobytes()
    assert run_profiles(case).tobytes() == table.tobytes()
    t3, s3 = run_profiles(case, return_shift=True)
    assert t3.tobytes() == table.tobytes() and s3.tobytes() == shifts.tobytes()


def by_input_position(case, cell_table):
    kept = np.flatnonzero(case["labels"] > 0)
    assert len(cell_table) == len(kept)
    assert np.array_equal(cell_table["cell"], case["cells"][kept]) and np.array_equal(cell_table["label"], case["labels"][kept])
    full = np.zeros(len(case["cells"]), dtype=cell_table.dtype)
    full[kept] = cell_table
    return full


@pytest.mark.parametrize("name", SNAMES)
def test_segments_against_the_restatement(name):
    case = scases()[SNAMES.index(name)]
    table, cells, curve, shifts = run_segments(case, return_cells=True, return_curve=True, return_shift=True)
    K, A = len(case["cells"]), len(case["ages"])
    assert cells.dtype.names[-3:] == ("shift_index", "shift", "label") and shifts.shape == (K, A) and shifts.dtype == np.int8
    # stage one: every d_ci of a usable cell against the single-profile restatement of that cell
    single = restate_profiles(case)
    ties = 0
    for k, r in enumerate(single):
        if r["usable"]:
            assert r["cond"] <= sh.COND_MAX, (r["cell"], r["cond"])
            ties += sh.check_shifts(r, shifts[k]) > 0
        else:
            assert not shifts[k].any()
    assert ties <= sh.TIE_SHARE * max(1, K), (ties, K)
    # stage two: the joint fit with those shifts
    ref = sh.fit_segments(case["z"], case["de"], case["cells"], case["labels"], case["angle"], case["h"], case["w"], case["D"],
                          case["ages"], shifts, case["delta"], case["min_samples"], case["min_profiles"])
    assert curve.shape == (len(ref), A)
    st = sh.compare_segments(ref, table, by_input_position(case, cells), curve, case["h"], case["de"], case["D"], case["delta"])
    print("%s: %s; cells with a shift decided inside the tolerance: %d" % (name, st, ties))
    extra = np.where(case["D"] > 0, table["n_profiles"], 0)
    assert np.array_equal(table["dof"], table["n"] - 2 * table["n_profiles"] - 1 - extra)
    if name == "sizes 1 2 64 65 300":
        assert sorted(table["n_profiles"]) == [1, 2, 64, 65, 300] and st["fitted"] == 5
    if name == "shuffled order":
        assert np.any(np.diff(case["labels"]) < 0) and st["fitted"] == len(table)
    if name == "unusable segment":
        assert list(table["label"]) == [4, 6] and list(table["n_profiles"]) == [0, 2] and list(table["status"] & 1) == [1, 0]
        assert table["n"][0] == 0 and table["dof"][0] == -1
    if name == "no cell":
        assert len(table) == 0 and len(cells) == 0
    # a second run, and the runs without the optional outputs: the same bytes
    t2, c2, v2, s2 = run_segments(case, return_cells=True, return_curve=True, return_shift=True)
    assert t2.tobytes() == table.tobytes() and c2.tobytes() == cells.tobytes() and v2.tobytes() == curve.tobytes()
    assert s2.tobytes() == shifts.tobytes()
    assert run_segments(case).tobytes() == table.tobytes()


def test_the_plane_of_a_segment_that_is_not_fitted():
    """Stage one does not know the segment: a usable cell keeps its d_ci in the plane when min_profiles leaves its
    segment without a fit, while the cell table, which speaks of the segment's best age, has shift_index 0 and NaN."""
    case = scases()[SNAMES.index("segments h30 w5 D4")]
    _, _, _, fitted_plane = run_segments(case, return_cells=True, return_curve=True, return_shift=True)
    table, cells, curve, plane = run_segments(dict(case, min_profiles=100), return_cells=True, return_curve=True,
                                              return_shift=True)
    assert (table["status"] == 1).all() and (table["n_profiles"] > 0).all() and (cells["used"] == 1).all()
    assert plane.tobytes() == fitted_plane.tobytes() and plane.any()
    assert not cells["shift_index"].any() and np.isnan(cells["shift"]).all() and np.isnan(curve).all()


# ---- the two anchors, as bytes ------------------------------------------------------------------------------------------
def same_bytes(a, b, fields):
    for f in fields:
        assert a[f].tobytes() == b[f].tobytes(), f


@pytest.mark.parametrize("name", ["synthetic h100 w5 D1", "synthetic h30 w5 D4", "64 ages", "borders and corners", "NaN cells"])
def test_a_range_of_zero_is_the_unshifted_call_profiles(name):
    case = pcases()[PNAMES.index(name)]
    base, bcurve = run_profiles(case, D=None, return_curve=True)
    zero, zcurve, zshift = run_profiles(case, D=0, return_curve=True, return_shift=True)
    assert "shift" not in base.dtype.names and (base["status"] != 1).sum() >= len(base) // 4
    same_bytes(zero, base, base.dtype.names)
    assert zcurve.tobytes() == bcurve.tobytes() and not zshift.any() and not zero["shift_index"].any()
    assert np.array_equal(np.isnan(zero["shift"]), zero["status"] == 1) and not np.nansum(np.abs(zero["shift"]))


@pytest.mark.parametrize("name", ["segments h100 w0 D8", "segments h30 w5 D4", "sizes 1 2 64 65 300", "unusable segment"])
def test_a_range_of_zero_is_the_unshifted_call_segments(name):
    case = scases()[SNAMES.index(name)]
    base, bcells, bcurve = run_segments(case, D=None, return_cells=True, return_curve=True)
    zero, zcells, zcurve, zshift = run_segments(case, D=0, return_cells=True, return_curve=True, return_shift=True)
    assert base.dtype == zero.dtype and zero.tobytes() == base.tobytes() and zcurve.tobytes() == bcurve.tobytes()
    same_bytes(zcells, bcells, bcells.dtype.names)
    assert not zshift.any() and not zcells["shift_index"].any()


def test_one_profile_segments_are_the_shifted_single_fit_byte_for_byte():
    for case in (pcases()[PNAMES.index(n)] for n in ("synthetic h100 w0 D8", "synthetic h30 w5 D4", "borders and corners",
                                                     "NaN cells", "D = h - min_samples")):
        K = len(case["cells"])
        lab = np.random.default_rng(3).permutation(K) + 1                  # one segment per cell, in shuffled order
        seg, ct, cv, sp = run_segments(case, labels=lab, return_cells=True, return_curve=True, return_shift=True)
        one, ocv, osp = run_profiles(case, return_curve=True, return_shift=True)
        assert sp.tobytes() == osp.tobytes()
        fit = one["status"] != 1
        assert fit.sum() >= K // 4
        for f in ("b", "c0", "sse", "shift_index", "shift", "cell", "n"):
            assert ct[f].tobytes() == one[f].tobytes(), (case["name"], f)
        one, ocv = one[np.argsort(lab)], ocv[np.argsort(lab)]              # in label order
        for f in ("kt_index", "lo_index", "hi_index", "status", "a", "sse", "rmse", "kt", "kt_lo", "kt_hi", "height"):
            assert seg[f].tobytes() == one[f].tobytes(), (case["name"], f)
        assert cv.tobytes() == ocv.tobytes()
        fit = one["status"] != 1
        assert np.array_equal(seg["dof"][fit], one["n"][fit] - 4) and (seg["n_cells"] == 1).all()


def test_matcher_routes_give_the_same_bytes():
    g = synthetic.synthetic_scarp(768, theta=0.6)
    m = sl.Matcher(g)
    m.search(sl.Scarp, 100., _plan.age_grid()[::5], _plan.angle_grid())
    res = np.array(m.result_array())
    lo, hi = np.percentile(res[3][res[3] > 0], [60, 90])
    tr = m.extract_traces(lo, hi, 4)
    cells = np.flatnonzero(tr.labels.ravel() > 0)
    assert len(cells) > 50 and len(tr.segments) > 1
    kw = dict(max_shift=4.0, return_curve=True, return_shift=True)
    a = m.fit_profiles(tr, 60., 3., **kw)
    b = sl.fit_profiles(g, cells, res[2], 60., 3., **kw)
    assert a[0].dtype.names[-1] == "label" and np.array_equal(a[0]["label"], tr.labels.ravel()[cells])
    same_bytes(a[0], b[0], b[0].dtype.names)
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and (b[0]["status"] != 1).sum() > 50
    assert m.fit_profiles(cells, 60., 3., max_shift=4.0).tobytes() == b[0].tobytes()
    a = m.fit_segments(tr, 60., 3., return_cells=True, **kw)
    b = sl.fit_segments(g, cells, tr.labels, res[2], 60., 3., return_cells=True, **kw)
    assert len(a) == 4 and all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and (a[0]["status"] != 1).sum() >= 1
    # the search's record is what it was
    assert np.array_equal(np.array(m.result_array()), res, equal_nan=True)


# ---- what it is for --------------------------------------------------------------------------------------------------------
def test_the_offset_case_on_the_device():
    """docs/segments.md: cells up to six columns off the line date the segment two grid steps too old; with the shift the
    joint fit returns the true index, no shift runs into the end of its range, and each is the offset seen along the
    profile."""
    z, cells, theta, off = sh.offset_case()
    g = grid(z, 1.0)
    lab = np.ones(len(cells), dtype=int)
    without = sl.fit_segments(g, cells, lab, theta, 100., 2.)[0]
    row, ct = sl.fit_segments(g, cells, lab, theta, 100., 2., max_shift=8.0, return_cells=True)
    row = row[0]
    print("joint: index %d [%d, %d] without the shift; %d [%d, %d] with, a %.5f, status %d; |d + offset cos(theta)| <= %.3f"
          % (without["kt_index"], without["lo_index"], without["hi_index"], row["kt_index"], row["lo_index"], row["hi_index"],
             row["a"], row["status"], np.abs(ct["shift_index"] + off * np.cos(theta)).max()))
    assert without["kt_index"] == 12 and row["kt_index"] == 10
    assert not row["status"] & 8 and row["n_profiles"] == 100 and row["dof"] == row["n"] - 301
    assert np.abs(ct["shift_index"] + off * np.cos(theta)).max() <= 1.5
    single = sl.fit_profiles(g, cells, theta, 100., 2., max_shift=8.0)
    assert not (single["status"] & 8).any() and np.abs(single["shift_index"] + off * np.cos(theta)).max() <= 1.5


def test_library_refuses_what_the_header_says(gpu_ctx):
    ctx = _lib.Context(0)
    z = pr.synthetic_z(64)
    ages = np.array([1.0, 2.0])
    i64, i32 = (lambda v: np.array(v, dtype=np.int64)), (lambda v: np.array(v, dtype=np.int32))
    cells, sa, ca = i64([5 * 64 + 30, 6 * 64 + 30]), np.zeros(2), np.ones(2)

    def prof(D, h=10, ms=4):
        return ctx.fit_profiles(cells, sa, ca, ages, h, 1, 1.0, 1.0, ms, z=z, shift=D)

    def segs(D, h=10, ms=4):
        return ctx.fit_segments(cells, sa, ca, i64([0, 1, 2]), i32([1, 2]), ages, h, 1, 1.0, 1.0, ms, 1, z=z, shift=D)
    for fn in (prof, segs):
        assert (fn(6)[0]["status"] & 1 == 0).all()                         # D = h - min_samples is the last one taken
        for kw in (dict(D=-1), dict(D=7), dict(D=5, ms=6)):
            with pytest.raises(_lib.ScarpletHipError, match=r"\(-1\)"):
                fn(**kw)
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\)"):
            fn(65, h=100)
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-3\)"):
        ctx.fit_profiles(cells, sa, ca, ages, 10, 1, 1.0, 1.0, 4, shift=2)  # no DEM set
    ctx.close()
