"""sl.fit_segments on the MI355X (sc_fit_segments / sc_fit_segments_dem, docs/segments.md) against the numpy
restatement (tests/segment_reference.py: one lstsq on the full design matrix per segment and age).

Tolerances are the project's (profile_reference.RTOL = 1e-9, COND_MAX = 1e3).  Every compared segment has a
column-scaled design matrix of condition number <= 1e3, asserted on the restatement.  sse within 1e-9 relative (the
whole curve, and each profile's share against the pooled sum); a, each c0 and each b h de within 1e-9 of the segment's
largest profile peak-to-peak range; n_cells, n_profiles, n, dof, status and used equal; kt_index, lo_index and hi_index
equal except where the restatement's own sse at the device's index is within 1e-9 relative of the value that decided -
such segments are counted, printed, and may be at most 1 % of a case's segments: none in a case of fewer than 100.
"""
import numpy as np
import pytest

import profile_reference as pr
import segment_reference as sr
import scarplet_amd as sl
from scarplet_amd import _lib, _plan, synthetic

pytestmark = pytest.mark.gpu


def grid(z, de):
    return sl.DEMGrid.from_array(z, float(de))


def run_case(case, **kw):
    h, w, de = case["h"], case["w"], case["de"]
    return sl.fit_segments(grid(case["z"], de), case["cells"], case["labels"], case["angle"], h * de, w * de,
                           ages=case["ages"], delta=case["delta"], min_samples=case["min_samples"],
                           min_profiles=case["min_profiles"], **kw)


def by_input_position(case, cell_table):
    """The cell table (input order of the kept cells) spread over the input positions, for segment_reference.compare."""
    kept = np.flatnonzero(case["labels"] > 0)
    assert len(cell_table) == len(kept)
    assert np.array_equal(cell_table["cell"], case["cells"][kept]) and np.array_equal(cell_table["label"], case["labels"][kept])
    nx = case["z"].shape[1]
    assert np.array_equal(cell_table["row"] * nx + cell_table["col"], cell_table["cell"])
    full = np.zeros(len(case["cells"]), dtype=cell_table.dtype)
    full[kept] = cell_table
    return full


def check_case(case):
    table, cells, curve = run_case(case, return_cells=True, return_curve=True)
    ref = sr.restate(case)
    S, A = len(ref), len(case["ages"])
    assert len(table) == S and curve.shape == (S, A)
    assert np.array_equal(table["label"], np.unique(case["labels"][case["labels"] > 0]))
    assert np.array_equal(table["height"], 2.0 * table["a"], equal_nan=True)
    st = sr.compare(ref, table, by_input_position(case, cells), curve, case["h"], case["de"], case["delta"])
    print("%s: %s; segments whose index was decided inside the tolerance: %d" % (case["name"], st, st["ties"]))
    fit = table["status"] != 1
    assert np.array_equal(table["dof"], table["n"] - 2 * table["n_profiles"] - 1)
    assert np.array_equal(table["rmse"][fit], np.sqrt(table["sse"][fit] / table["dof"][fit]))
    assert np.array_equal(table["kt"][fit], case["ages"][table["kt_index"][fit]])
    assert np.array_equal(table["kt_lo"][fit], case["ages"][table["lo_index"][fit]])
    assert np.array_equal(table["kt_hi"][fit], case["ages"][table["hi_index"][fit]])
    assert np.array_equal(curve[fit, table["kt_index"][fit]], table["sse"][fit])
    # a second run, and the runs without the optional outputs: the same bytes
    t2, c2, v2 = run_case(case, return_cells=True, return_curve=True)
    assert t2.tobytes() == table.tobytes() and c2.tobytes() == cells.tobytes() and v2.tobytes() == curve.tobytes()
    assert run_case(case).tobytes() == table.tobytes()
    t3, c3 = run_case(case, return_cells=True)
    assert t3.tobytes() == table.tobytes() and c3.tobytes() == cells.tobytes()
    return table, cells, curve, ref, st


CASES = None


def cases():
    global CASES
    if CASES is None:
        CASES = sr.gpu_cases()
    return CASES


NAMES = ["synthetic h100 w0", "synthetic h100 w5", "synthetic h30 w5", "synthetic h15 w2", "sizes 1 2 64 65 2100",
         "shuffled order", "repeated cells", "one age", "64 ages", "min_profiles 25", "no cell", "labels <= 0 only",
         "borders", "unusable segment", "NaN cells"]


def test_the_case_list_is_the_one_named_here():
    assert [c["name"] for c in cases()] == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_against_the_restatement(name):
    case = cases()[NAMES.index(name)]
    table, cells, curve, ref, st = check_case(case)
    if name == "sizes 1 2 64 65 2100":
        assert sorted(table["n_profiles"]) == [1, 2, 64, 65, 2100] and st["fitted"] == 5
    if name == "shuffled order":
        assert np.any(np.diff(case["labels"]) < 0) and st["fitted"] == len(table)
    if name in ("borders", "NaN cells"):
        assert (table["n_profiles"] < table["n_cells"]).any() or name == "NaN cells"
        full = np.array([r["n_profiles"] * (2 * case["h"] + 1) for r in ref])
        assert (table["n"][table["status"] != 1] < full[table["status"] != 1]).sum() >= 5     # fitted with points missing
    if name == "unusable segment":
        assert list(table["label"]) == [4, 6] and list(table["n_profiles"]) == [0, 2] and list(table["status"] & 1) == [1, 0]
        assert list(table["n_cells"]) == [4, 2] and table["n"][0] == 0 and table["dof"][0] == -1
    if name == "min_profiles 25":
        assert (table["status"] == 1).all() and (table["n_profiles"] > 0).all() and (cells["used"] == 1).all()
    if name in ("no cell", "labels <= 0 only"):
        assert len(table) == 0 and len(cells) == 0 and curve.shape == (0, len(case["ages"]))
    if name == "repeated cells":
        for k in range(0, 21, 3):
            assert cells[k:k + 3].tobytes() == cells[k:k + 1].tobytes() * 3


def trace_case(name):
    """A real search on a golden crop, its traces, and the joint fit of every segment through the Matcher."""
    z, de = pr._golden_dem(name)
    ages = _plan.age_grid()
    m = sl.Matcher(grid(z, de))
    res = np.array(m.search(sl.Scarp, 100., ages[::5], _plan.angle_grid()).result_array())
    s = res[3][res[3] > 0]
    lo, hi = np.percentile(s, 90), np.percentile(s, 99)
    tr = m.extract_traces(lo, hi, 8)
    return m, res, tr, z, de


@pytest.mark.parametrize("name, h, w", [("dem_carrizo.npz", 25, 2), ("dem_grandcanyon.npz", 30, 1)])
def test_traces_of_a_real_search(name, h, w):
    m, res, tr, z, de = trace_case(name)
    kt = _plan.age_grid()[:21:4]                                          # 1 .. 100: bent over a profile of 50 data units
    assert len(tr.segments) >= 5
    cells = np.flatnonzero(tr.labels.ravel() > 0)
    print("%s: %d segments, %d cells, the largest %d" % (name, len(tr.segments), len(cells), tr.segments["n_cells"].max()))
    case = dict(name=name, z=z, de=de, cells=cells, labels=tr.labels.ravel()[cells].astype(np.int64), angle=res[2].ravel()[cells],
                h=h, w=w, ages=kt, delta=1.0, min_samples=8, min_profiles=1)
    table, ct, curve, ref, st = check_case(case)
    assert st["fitted"] >= 5
    # the Matcher route: the DEM on the device, the same bytes, one row per row of the traces' table
    mt, mc, mv = m.fit_segments(tr, h * de, w * de, ages=kt, min_samples=8, return_cells=True, return_curve=True)
    assert mt.tobytes() == table.tobytes() and mc.tobytes() == ct.tobytes() and mv.tobytes() == curve.tobytes()
    assert np.array_equal(mt["label"], tr.segments["label"]) and np.array_equal(mt["n_cells"], tr.segments["n_cells"])


def test_one_cell_segments_are_fit_profiles_byte_for_byte():
    for case in (cases()[NAMES.index(n)] for n in ("synthetic h100 w5", "synthetic h15 w2", "borders", "NaN cells", "64 ages")):
        K = len(case["cells"])
        lab = np.random.default_rng(3).permutation(K) + 1                  # one segment per cell, in shuffled order
        h, w, de = case["h"], case["w"], case["de"]
        kw = dict(ages=case["ages"], delta=case["delta"], min_samples=case["min_samples"])
        seg, ct, cv = sl.fit_segments(grid(case["z"], de), case["cells"], lab, case["angle"], h * de, w * de, return_cells=True,
                                      return_curve=True, **kw)
        one, ocv = sl.fit_profiles(grid(case["z"], de), case["cells"], case["angle"], h * de, w * de, return_curve=True, **kw)
        one, ocv = one[np.argsort(lab)], ocv[np.argsort(lab)]                       # in label order
        assert (one["status"] != 1).sum() >= K // 4
        for f in ("kt_index", "lo_index", "hi_index", "status", "a", "sse", "rmse", "kt", "kt_lo", "kt_hi", "height"):
            assert seg[f].tobytes() == one[f].tobytes(), (case["name"], f)
        assert cv.tobytes() == ocv.tobytes()
        fit = one["status"] != 1
        assert np.array_equal(seg["n_profiles"], fit.astype(np.int32)) and np.array_equal(seg["dof"][fit], one["n"][fit] - 3)
        assert (seg["n_cells"] == 1).all()
        # the cell table, in input order: the profile's own slope and intercept
        back = one[np.argsort(np.argsort(lab))]
        for f in ("cell", "n", "b", "c0", "sse"):
            assert ct[f].tobytes() == back[f].tobytes(), (case["name"], f)


def test_noisy_surface_on_the_device():
    z, cells, theta = sr.noisy_case()
    g = grid(z, 1.0)
    row = sl.fit_segments(g, cells, np.ones(100, dtype=int), theta, 100., 2.)[0]
    single = sl.fit_profiles(g, cells, theta, 100., 2.)
    print("joint: index %d, interval [%d, %d], a %.5f; single cells: %d of 100 on index 10"
          % (row["kt_index"], row["lo_index"], row["hi_index"], row["a"], (single["kt_index"] == 10).sum()))
    assert row["kt_index"] == 10 and row["lo_index"] == 10 and row["hi_index"] == 10
    assert row["n_profiles"] == 100 and row["n"] == 20100 and row["dof"] == 19899
    assert (single["kt_index"] == 10).sum() <= 30


def test_matcher_route_gives_the_same_bytes_and_leaves_the_search_alone():
    g = synthetic.synthetic_scarp(768, theta=0.6)
    m = sl.Matcher(g)
    m.search(sl.Scarp, 100., _plan.age_grid()[::5], _plan.angle_grid())
    before = np.array(m.result_array())
    lo, hi = np.percentile(before[3][before[3] > 0], [60, 90])
    tr0 = m.extract_traces(lo, hi, 4)
    cells = np.flatnonzero(tr0.labels.ravel() > 0)
    assert len(cells) > 50 and len(tr0.segments) > 1
    a, ac, av = m.fit_segments(tr0, 60., 3., return_cells=True, return_curve=True)
    assert np.array_equal(a["label"], tr0.segments["label"]) and np.array_equal(a["n_cells"], tr0.segments["n_cells"])
    assert np.array_equal(ac["cell"], cells) and np.array_equal(ac["label"], tr0.labels.ravel()[cells])
    b, bc, bv = sl.fit_segments(g, cells, tr0.labels, before[2], 60., 3., return_cells=True, return_curve=True)
    c = sl.fit_segments(g, tr0.labels > 0, tr0.labels.ravel()[cells], before[2].ravel()[cells], 60., 3.)
    assert a.tobytes() == b.tobytes() == c.tobytes() and ac.tobytes() == bc.tobytes() and av.tobytes() == bv.tobytes()
    assert (a["status"] != 1).sum() >= 1
    # strike="segment": every cell of a segment cut across that segment's strike
    d = m.fit_segments(tr0, 60., 3., strike="segment")
    e = sl.fit_segments(g, cells, tr0.labels, tr0.segments["strike"][tr0.labels.ravel()[cells] - 1], 60., 3.)
    assert d.tobytes() == e.tobytes() and np.array_equal(d["label"], tr0.segments["label"])
    assert d.tobytes() != a.tobytes()
    # the search's record, its planes and the traces are what they were
    assert np.array_equal(np.array(m.result_array()), before, equal_nan=True)
    tr1 = m.extract_traces(lo, hi, 4)
    assert np.array_equal(tr0.labels, tr1.labels) and tr0.segments.tobytes() == tr1.segments.tobytes()
    again = np.array(m.search(sl.Scarp, 100., _plan.age_grid()[::5], _plan.angle_grid()).result_array())
    assert np.array_equal(again, before, equal_nan=True)


def test_library_refuses_what_the_header_says(gpu_ctx):
    ctx = _lib.Context(0)
    z = pr.synthetic_z(64)
    ages = np.array([1.0, 2.0])
    i64, i32 = (lambda v: np.array(v, dtype=np.int64)), (lambda v: np.array(v, dtype=np.int32))
    base = dict(cells=i64([5 * 64 + 30, 6 * 64 + 30]), sa=np.array([0.0, 0.0]), ca=np.array([1.0, 1.0]), start=i64([0, 1, 2]),
                label=i32([1, 2]), kt=ages, h=10, w=1, de=1.0, delta=1.0, ms=4, mp=1, zz=z)

    def fit(**kw):
        a = dict(base, **kw)
        return ctx.fit_segments(a["cells"], a["sa"], a["ca"], a["start"], a["label"], a["kt"], a["h"], a["w"], a["de"],
                                a["delta"], a["ms"], a["mp"], cell_table=True, curve=True, z=a["zz"])
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-3\)"):
        fit(zz=None)                                                       # no DEM set
    rows, ct, cv = fit()
    assert list(rows["label"]) == [1, 2] and (rows["status"] != 1).all() and (ct["used"] == 1).all()
    for kw in (dict(cells=i64([64 * 64, 5])), dict(sa=np.array([np.nan, 0.0])), dict(kt=np.array([2.0, 1.0])), dict(ms=1),
               dict(ms=11), dict(delta=-1.0), dict(zz=z[:1].copy()), dict(de=0.0),
               dict(start=i64([0, 2, 1])), dict(start=i64([1, 1, 2])), dict(start=i64([0, 1, 1])), dict(start=i64([0, 1, 3])),
               dict(label=i32([0, 1])), dict(label=i32([-2, 1])), dict(label=i32([2, 2])), dict(label=i32([3, 2])), dict(mp=0)):
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-1\)"):
            fit(**kw)
    for kw in (dict(kt=np.arange(1.0, 66.0)), dict(h=1025), dict(w=33)):
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\)"):
            fit(**kw)
    # the largest supported call: a segment whose parked profiles pass SC_SEGMENT_MAX_PARK bytes
    h, A = 1024, 64
    big = _lib.SEGMENT_MAX_PARK // (8 * ((2 * h + 1) + 4 * A)) + 1
    kt = 10 ** np.linspace(0, 3, A)
    many = dict(cells=np.full(big, 2080, dtype=np.int64), sa=np.zeros(big), ca=np.ones(big), kt=kt, h=h)
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\)"):
        fit(start=i64([0, big]), label=i32([1]), **many)
    with pytest.raises(ValueError, match="a segment of"):
        sl.fit_segments(grid(z, 1.0), many["cells"], np.ones(big, dtype=int), 0.0, float(h), ages=kt)
    # empty segments are rows without a fit
    rows, ct, cv = fit(start=i64([0, 0, 2]))
    assert list(rows["n_cells"]) == [0, 2] and list(rows["status"] & 1) == [1, 0] and np.isnan(cv[0]).all()
    # a context that holds a block of a larger grid
    zb = np.ascontiguousarray(z[:40, :])
    ax = np.arange(64.0)
    ctx.set_dem(zb, 1.0, 1.0, ax, ax, origin=(0, 0), shape=(64, 64), core=(0, 32, 0, 64), wrap=False)
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\)"):
        fit(zz=None)
    ctx.close()
