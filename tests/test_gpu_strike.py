"""sl.fit_along_strike on the MI355X (sc_fit_strike, docs/strike.md) against the numpy restatement
(tests/strike_reference.py): one lstsq per window and age on the full design matrix.

Integers - label, station, n_cells, n_profiles, n, dof - match exactly.  A kt_index, lo_index or hi_index that differs
from the restatement's must have been decided within 1e-9 relative by the restatement's own curve
(segment_reference.compare's rule); such windows may be at most 1 % of a case.  a agrees within 1e-9 of the profiles'
peak-to-peak range, sse and the curve within 1e-9 relative.  The ground the tolerances stand on is asserted on the
restatement: condition number <= 1e3 and SSpp / sse_min <= 1e3 in every compared window (the device forms sse_i as
SSpp - Q_i, docs/strike.md "The subtraction").  The anchors and the independence of segments are byte comparisons."""
import numpy as np
import pytest

import shift_reference as sh
import strike_reference as stk
import scarplet_amd as sl
from scarplet_amd import _plan, synthetic

pytestmark = pytest.mark.gpu

CASES = REFS = None
NAMES = ["noisy 30 15", "noisy 60 30", "noisy 9 9", "noisy 400 400", "run 1", "run 63", "run 64", "run 65", "run 128",
         "run 129", "run 130", "one age", "64 ages", "unusable", "unusable min_profiles 3", "several segments", "D 3"]


def cases():
    global CASES
    if CASES is None:
        CASES = {c["name"]: c for c in stk.gpu_cases()}
    return CASES


def grid(z):
    return sl.DEMGrid.from_array(z, 1.0)


def run(case, cells=None, labels=None, angle=None, **kw):
    args = dict(window=case["window"], step=case["step"], ages=case["ages"], delta=case["delta"],
                min_samples=case["min_samples"], min_profiles=case["min_profiles"],
                max_shift=float(case["D"]) if case["D"] else None)
    args.update(kw)
    return sl.fit_along_strike(grid(case["z"]), case["cells"] if cells is None else cells,
                               case["labels"] if labels is None else labels, case["angle"] if angle is None else angle,
                               float(case["h"]), float(case["w"]), **args)


def device_shifts(case):
    """Stage one's d_ci in input order (the (K, A) plane of fit_segments on the same cells), each entry checked against
    the single-profile restatement first, as tests/test_gpu_shift.py does."""
    plane = sl.fit_segments(grid(case["z"]), case["cells"], case["labels"], case["angle"], float(case["h"]), float(case["w"]),
                            ages=case["ages"], min_samples=case["min_samples"], max_shift=float(case["D"]),
                            return_shift=True)[1]
    single = sh.fit_profiles(case["z"], 1.0, case["cells"], case["angle"], case["h"], case["w"], case["D"], case["ages"],
                             case["delta"], case["min_samples"])
    ties = 0
    for k, r in enumerate(single):
        if r["usable"]:
            assert r["cond"] <= sh.COND_MAX, (r["cell"], r["cond"])
            ties += sh.check_shifts(r, plane[k]) > 0
        else:
            assert not plane[k].any()
    assert ties <= sh.TIE_SHARE * max(1, len(single)), ties
    return plane


def ref_of(name, shifts=None):
    """The restatement of a case, computed once and left unchanged."""
    global REFS
    REFS = REFS or {}
    if name not in REFS:
        REFS[name] = stk.restate(cases()[name], shifts)
    return REFS[name]


def test_the_case_list_is_the_one_named_here():
    assert list(cases()) == NAMES
    for c in cases().values():
        assert max(c["z"].shape) <= 600 and len(c["cells"]) <= 300
    c = cases()["noisy 30 15"]
    assert len(c["cells"]) == 100 and c["h"] == 100 and c["w"] == 2 and np.array_equal(c["ages"], _plan.age_grid())


@pytest.mark.parametrize("name", NAMES)
def test_against_the_restatement(name):
    case = cases()[name]
    table, curve = run(case, return_curve=True)
    A = len(case["ages"])
    assert curve.shape == (len(table), A) and curve.dtype == np.float64
    ref = ref_of(name, device_shifts(case) if case["D"] else None)
    st = stk.compare(ref, table, curve, case["ages"], case["delta"])
    print("%s: %s" % (name, st))
    prof = table["n_profiles"]
    if name.startswith("noisy"):
        assert len(table) == {"noisy 30 15": 21, "noisy 60 30": 11, "noisy 9 9": 34, "noisy 400 400": 1}[name]
        assert st["fitted"] == len(table) and st["ties"] == 0              # (the restatement alone needs no excuse: CPU)
    if name == "noisy 400 400":
        assert prof.tolist() == [100] and table["kt_index"][0] == 10       # one window over everything: docs/segments.md
    if name.startswith("run"):
        assert int(name.split()[1]) in prof.tolist(), prof
    if name == "one age":
        assert A == 1 and (table["status"] == 6).all() and (table["kt_index"] == 0).all()
    if name == "64 ages":
        assert A == 64
    if name.startswith("unusable"):
        cells_of = table["n_cells"]
        assert ((cells_of == 0) & (table["status"] == 1)).any()           # an empty window
        assert ((cells_of > 0) & (prof == 0)).any()                        # cells, none usable
        assert ((prof > 0) & (prof < cells_of) & (table["status"] != 1)).any()          # some unusable in a run
        assert np.isnan(table["row"][cells_of == 0]).all() and not np.isnan(table["row"][cells_of > 0]).any()
        sparse = (prof > 0) & (prof < 3)
        assert sparse.any() and ((table["status"][sparse] == 1) == (case["min_profiles"] == 3)).all()
        assert sorted(set(table["label"].tolist())) == [3, 7]
    if name == "several segments":
        assert sorted(set(table["label"].tolist())) == [2, 5, 9, 11] and np.any(np.diff(case["labels"]) < 0)
        one = table[table["label"] == 11]
        assert len(one) == 1 and one["n_cells"][0] == 1 and one["station"][0] == 0
    if name == "D 3":
        extra = table["n_profiles"]
        assert np.array_equal(table["dof"], table["n"] - 3 * extra - 1)
    # the table is sorted by (label, station)
    key = table["label"].astype(np.int64) * (1 << 32) + table["station"]
    assert (np.diff(key) > 0).all()
    # a second run and the run without the curve: the same bytes
    t2, c2 = run(case, return_curve=True)
    assert t2.tobytes() == table.tobytes() and c2.tobytes() == curve.tobytes()
    assert run(case).tobytes() == table.tobytes()


def test_a_segment_does_not_depend_on_the_others():
    """Each segment's rows are the same bytes whether it is passed alone or with the others, in shuffled order."""
    case = cases()["several segments"]
    table, curve = run(case, return_curve=True)
    for L in np.unique(table["label"]):
        pick = case["labels"] == L
        t1, c1 = run(case, cells=case["cells"][pick], labels=case["labels"][pick], angle=case["angle"][pick],
                     return_curve=True)
        rows = table["label"] == L
        assert t1.tobytes() == table[rows].tobytes() and c1.tobytes() == curve[rows].tobytes(), L


# ---- the anchors, as bytes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [None, 3.0])
def test_one_window_over_a_segment_is_fit_segments(D):
    """A window that holds the whole segment, whose input order is its order along the strike: the sums have the shape
    of fit_segments' - runs of 64 from the first usable profile - so a is bit for bit fit_segments', and the argmax of Q
    is its kt_index.  200 cells: four runs."""
    case = cases()["run 130"]
    assert (np.diff(case["cells"]) > 0).all()
    g = grid(case["z"])
    kw = dict(ages=case["ages"], min_samples=case["min_samples"], max_shift=D)
    row = sl.fit_along_strike(g, case["cells"], case["labels"], case["angle"], 20.0, 1.0, window=400.0, step=400.0, **kw)
    fit = sl.fit_segments(g, case["cells"], case["labels"], case["angle"], 20.0, 1.0, **kw)
    assert len(row) == 1 and len(fit) == 1 and row["n_profiles"][0] == 200 and fit["status"][0] != 1
    for f in ("label", "n_cells", "n_profiles", "n", "dof", "kt_index", "kt"):
        assert row[f].tobytes() == fit[f].tobytes(), f
    assert row["a"].tobytes() == fit["a"].tobytes() and row["height"].tobytes() == fit["height"].tobytes()
    assert abs(row["sse"][0] - fit["sse"][0]) <= 1e-9 * fit["sse"][0]
    assert (row["status"][0] & 8) == (fit["status"][0] & 8)


@pytest.mark.parametrize("D", [None, 3.0])
def test_a_window_of_one_profile_is_fit_profiles(D):
    """Windows of one cell each (window = step = the cell size on a column): kt_index and a are fit_profiles' for that
    cell, bit for bit - one profile is no addition at all."""
    case = cases()["run 1"]
    g = grid(case["z"])
    kw = dict(ages=case["ages"], min_samples=case["min_samples"], max_shift=D)
    table = sl.fit_along_strike(g, case["cells"], case["labels"], case["angle"], 20.0, 1.0, window=1.0, step=1.0, **kw)
    one = sl.fit_profiles(g, case["cells"], case["angle"], 20.0, 1.0, **kw)
    assert len(table) == 200 and (table["n_profiles"] == 1).all() and (one["status"] != 1).all()
    assert np.array_equal(table["row"] * case["z"].shape[1] + table["col"], case["cells"])
    assert table["kt_index"].tobytes() == one["kt_index"].tobytes() and table["a"].tobytes() == one["a"].tobytes()
    assert np.array_equal(table["n"], one["n"]) and np.array_equal(table["dof"], one["n"] - (4 if D else 3))
    assert (np.abs(table["sse"] - one["sse"]) <= 1e-9 * one["sse"]).all()
    if D:
        assert np.array_equal(table["status"] & 8, one["status"] & 8)


# ---- determinism and routes ---------------------------------------------------------------------------------------------
def test_both_strike_modes_through_the_matcher():
    """A real search, its traces, and the windows of every segment through the Matcher: the bytes of the free function
    with the same orientations, with strike="cell" and with strike="segment"."""
    g = synthetic.synthetic_scarp(768, theta=0.6)
    m = sl.Matcher(g)
    m.search(sl.Scarp, 100., _plan.age_grid()[::5], _plan.angle_grid())
    res = np.array(m.result_array())
    lo, hi = np.percentile(res[3][res[3] > 0], [60, 90])
    tr = m.extract_traces(lo, hi, 4)
    cells = np.flatnonzero(tr.labels.ravel() > 0)
    assert len(cells) > 50 and len(tr.segments) > 1
    a, ca = m.fit_along_strike(tr, 60., 40., step=10., swath=3., return_curve=True)
    b, cb = sl.fit_along_strike(g, cells, tr.labels, res[2], 60., 3., window=40., step=10., return_curve=True)
    assert a.tobytes() == b.tobytes() and ca.tobytes() == cb.tobytes() and (a["status"] != 1).sum() >= 1
    assert np.array_equal(np.unique(a["label"]), tr.segments["label"])
    d = m.fit_along_strike(tr, 60., 40., step=10., swath=3., strike="segment", max_shift=2.0)
    e = sl.fit_along_strike(g, cells, tr.labels, tr.segments["strike"][tr.labels.ravel()[cells] - 1], 60., 3., window=40.,
                            step=10., max_shift=2.0)
    assert d.tobytes() == e.tobytes() and d.tobytes() != a.tobytes()
    # the search's record is what it was
    assert np.array_equal(np.array(m.result_array()), res, equal_nan=True)


def test_library_refuses_what_the_header_says(gpu_ctx):
    from scarplet_amd import _lib
    import profile_reference as pr
    ctx = _lib.Context(0)
    z = pr.synthetic_z(64)
    ages = np.array([1.0, 2.0])
    i64, i32 = (lambda v: np.array(v, dtype=np.int64)), (lambda v: np.array(v, dtype=np.int32))
    cells, sa, ca = i64([5 * 64 + 30, 6 * 64 + 30, 7 * 64 + 30]), np.zeros(3), np.ones(3)

    def fit(sws=(0, 1, 2), lo=(0, 2), hi=(2, 3), D=0, seg=(0, 2, 3)):
        return ctx.fit_strike(cells, sa, ca, i64(seg), i32([1, 2]), i64(sws), i64(lo), i64(hi), ages, 10, 1, D, 1.0, 1.0, 4,
                              1, z=z)[0]
    ok = fit()
    assert ok["n_cells"].tolist() == [2, 1] and (ok["status"] & 1 == 0).all() and ok["station"].tolist() == [0, 0]
    assert fit(lo=(1, 3), hi=(1, 3))["n_cells"].tolist() == [0, 0]         # empty windows are allowed
    for kw in (dict(lo=(0, 1)), dict(hi=(3, 3)), dict(lo=(2, 2), hi=(1, 3)), dict(sws=(0, 1, 1)), dict(sws=(1, 1, 2)),
               dict(sws=(0, 2, 1)), dict(D=-1), dict(D=7), dict(seg=(0, 2, 2))):
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-1\)"):
            fit(**kw)
    ctx.close()
