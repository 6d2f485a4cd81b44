"""sl.fit_segments(refine=R) on the MI355X (sc_fit_segments_refine / sc_fit_segments_refine_dem; docs/segments.md,
"Continuous ages") against the numpy restatement (tests/segment_refine_reference.py).

What is compared, and where the tolerances come from.
* The shared fields of the row and of the cell table, and the curves, are the plain call's bytes: no tolerance.  With
  refine=0 every fine field is its grid counterpart's bytes, and a segment of one usable profile returns the bytes of
  sl.fit_profiles(refine=R) for that cell.
* sse_fine is within 1e-9 relative of float64 lstsq (ONE solve on the full design matrix) at the device's own kt_fine,
  unconditionally; a_fine and each profile's b_fine h de and c0_fine are within 1e-9 of the profiles' range, each profile's
  sse_fine within 1e-9 of the pooled sse: the tolerances of tests/test_gpu_segments.py, on the same condition - every compared
  design matrix, the candidates' included, has a column-scaled condition number <= 1e3, asserted on the restatement.
* kt_fine, kt_lo_fine, kt_hi_fine and status_fine are bit-equal to the restatement's, except where the decision that parted
  was taken inside 1e-9 relative (the margins of tests/refine_reference.py, on the pooled sse).  Such segments are counted
  and may be at most 1 % of a case: none in every case under 100 segments.  On these inputs float64 lstsq and longdouble
  per-profile orthogonalisation part in no segment, and the segments with a margin below 1e-8 stay within the same cap
  (tests/test_segment_refine_host.py).
"""
import numpy as np
import pytest

import segment_refine_reference as sx
import scarplet_amd as sl
from scarplet_amd import _lib, _plan, segments, synthetic

pytestmark = pytest.mark.gpu

SHARED = segments.FIT_DTYPE.names
SHARED_CELL = segments.CELL_DTYPE.names
FINE = ("kt_fine", "kt_lo_fine", "kt_hi_fine", "a_fine", "sse_fine", "rmse_fine", "height_fine", "status_fine")
GRID_OF = dict(kt_fine="kt", kt_lo_fine="kt_lo", kt_hi_fine="kt_hi", a_fine="a", sse_fine="sse", rmse_fine="rmse",
               height_fine="height", status_fine="status")
CELL_GRID_OF = dict(b_fine="b", c0_fine="c0", sse_fine="sse")


def grid(z, de):
    return sl.DEMGrid.from_array(z, float(de))


def run_case(case, refine, return_cells=True, return_curve=True):
    h, w, de = case["h"], case["w"], case["de"]
    return sl.fit_segments(grid(case["z"], de), case["cells"], case["labels"], case["angle"], h * de, w * de, ages=case["ages"],
                           delta=case["delta"], min_samples=case["min_samples"], min_profiles=case["min_profiles"],
                           return_cells=return_cells, return_curve=return_curve, refine=refine)


def by_position(case, cell_table):
    """The cell table (in input order of the kept cells) indexed by input position."""
    kept = np.flatnonzero(case["labels"] > 0)
    full = np.zeros(len(case["labels"]), dtype=cell_table.dtype)
    full[kept] = cell_table
    return full


def test_the_case_list_is_the_one_named_here():
    assert [c["name"] for c in sx.gpu_cases()] == sx.NAMES == [
        "synthetic", "sizes 1 2 64 65 130", "one age", "64 ages", "best age below the grid", "best age above the grid",
        "min_profiles 25", "unusable segment", "no cell", "labels <= 0 only", "NaN cells and borders", "shuffled order",
        "repeated cells", "120 segments of 3", "h1024"]


@pytest.mark.parametrize("R", sx.LEVELS)
@pytest.mark.parametrize("name", sx.NAMES)
def test_against_the_restatement(name, R):
    case = sx.gpu_cases()[sx.NAMES.index(name)]
    ref = sx.reference(name, R)
    S, A, K = len(ref), len(case["ages"]), int((case["labels"] > 0).sum())
    table, cells, curve = run_case(case, R)
    assert table.dtype.names == SHARED + FINE and len(table) == S and curve.shape == (S, A)
    assert cells.dtype.names == SHARED_CELL[:-1] + sx.CELL_FLOATS + ("label",) and len(cells) == K
    # anchor 1: refine=None is the plain call, and the shared fields and the curves are its bytes
    plain, pcells, pcurve = run_case(case, None)
    assert plain.dtype == segments.FIT_DTYPE and pcells.dtype == segments.CELL_DTYPE
    for f in SHARED:
        assert table[f].tobytes() == plain[f].tobytes(), f
    for f in SHARED_CELL:
        assert cells[f].tobytes() == pcells[f].tobytes(), f
    assert curve.tobytes() == pcurve.tobytes()
    # anchor 2: no level: every fine field is its grid counterpart
    zero, zcells, zcurve = run_case(case, 0)
    assert zero.dtype == table.dtype and zcells.dtype == cells.dtype and zcurve.tobytes() == pcurve.tobytes()
    for f, g in GRID_OF.items():
        assert zero[f].tobytes() == plain[g].astype(zero[f].dtype).tobytes(), f
    for f, g in CELL_GRID_OF.items():
        assert zcells[f].tobytes() == pcells[g].tobytes(), f
    # the restatement
    st = sx.compare(ref, sx.device_rows(table, by_position(case, cells), ref), case, R)
    print("%s, R = %d: %s" % (name, R, st))
    # structure (per segment in compare; here what concerns the tables as a whole)
    fit = table["status"] != 1
    assert np.all(table["sse_fine"][fit] <= table["sse"][fit])
    assert np.all((table["kt_lo_fine"][fit] <= table["kt_fine"][fit]) & (table["kt_fine"][fit] <= table["kt_hi_fine"][fit]))
    assert np.array_equal(table["rmse_fine"][fit], np.sqrt(table["sse_fine"][fit] / table["dof"][fit]))
    assert np.array_equal(table["height_fine"], 2.0 * table["a_fine"], equal_nan=True)
    assert np.all(table["status_fine"][~fit] == 1) and np.all((table["status_fine"][fit] & ~6) == 0)
    for f in FINE[:-1]:
        assert np.isnan(table[f][~fit]).all() and not np.isnan(table[f][fit]).any(), f
    for f in sx.CELL_FLOATS:
        assert np.array_equal(np.isnan(cells[f]), np.isnan(cells["b"])), f
    # anchor 4: a fine age that is a grid age has the grid fit's bits, in the row and in the cell table
    on = fit & (table["kt_fine"] == table["kt"])
    for f, g in (("sse_fine", "sse"), ("a_fine", "a")):
        assert table[f][on].tobytes() == table[g][on].tobytes(), f
    con = np.isin(cells["label"], table["label"][on])
    for f, g in CELL_GRID_OF.items():
        assert cells[f][con].tobytes() == cells[g][con].tobytes(), f
    if name in ("synthetic", "64 ages", "120 segments of 3", "NaN cells and borders"):
        assert (fit & (table["kt_fine"] != table["kt"])).any()
    if name == "sizes 1 2 64 65 130":
        assert sorted(table["n_profiles"]) == [1, 2, 64, 65, 130] and fit.all()
    if name == "best age below the grid":
        assert np.all(table["kt_index"] == 0) and np.all(table["status_fine"] & 2 > 0)
    if name == "best age above the grid":
        assert np.all(table["kt_index"] == A - 1) and np.all(table["status_fine"] & 4 > 0)
    if name == "one age":
        assert np.all(table["kt_fine"] == case["ages"][0]) and np.all(table["status_fine"] == 6)
    if name in ("min_profiles 25", "unusable segment"):
        assert fit.any() and (~fit).any()
    if name in ("no cell", "labels <= 0 only"):
        assert S == 0 and K == 0
    if name == "NaN cells and borders":
        assert (cells["used"] == 0).any() and ((cells["used"] == 1) & (cells["n"] < 2 * case["h"] + 1)).sum() >= 5
    # a second run, and a run without the cell table and the curve: the same bytes
    again = run_case(case, R)
    assert again[0].tobytes() == table.tobytes() and again[1].tobytes() == cells.tobytes() and again[2].tobytes() == curve.tobytes()
    assert run_case(case, R, return_cells=False, return_curve=False).tobytes() == table.tobytes()


@pytest.mark.parametrize("R", sx.LEVELS)
def test_a_segment_of_one_profile_is_fit_profiles_refine(R):
    """Anchor 3, on the cells of "synthetic", each as its own segment."""
    case = sx.gpu_cases()[sx.NAMES.index("synthetic")]
    K = len(case["cells"])
    one = dict(case, labels=np.arange(1, K + 1))
    table, cells, curve = run_case(one, R)
    h, w, de = case["h"], case["w"], case["de"]
    prof, pcurve = sl.fit_profiles(grid(case["z"], de), case["cells"], case["angle"], h * de, w * de, ages=case["ages"],
                                   delta=case["delta"], min_samples=case["min_samples"], return_curve=True, refine=R)
    assert (prof["status"] != 1).all() and (prof["kt_fine"] != prof["kt"]).sum() > K // 2
    for f in ("kt_fine", "kt_lo_fine", "kt_hi_fine", "a_fine", "sse_fine", "rmse_fine", "status_fine", "height_fine"):
        assert table[f].tobytes() == prof[f].tobytes(), f
    for f in ("b_fine", "c0_fine"):
        assert cells[f].tobytes() == prof[f].tobytes(), f
    assert cells["sse_fine"].tobytes() == prof["sse_fine"].tobytes() and curve.tobytes() == pcurve.tobytes()


def launches_of(R, cells):
    """The launches of one chunk (docs/segments.md, "Continuous ages"): 10 + 14 R, or 4 for a chunk without cells."""
    return 10 + 14 * R if cells else 4


def test_in_many_chunks_the_same_bytes_and_the_documented_launches():
    """The option "fit_chunk" bounds this call's chunks of whole segments: on a context of its own, through the binding (the
    raw rows, padding included), on an uploaded DEM.  The launches depend on R and on the chunks alone, never on the data."""
    c = sx.gpu_cases()[sx.NAMES.index("NaN cells and borders")]
    a = segments.check_args(c["z"].shape, c["de"], c["cells"], c["labels"], c["angle"], c["h"] * c["de"], c["w"] * c["de"],
                            c["ages"], c["delta"], c["min_samples"], c["min_profiles"])[:12]
    z = np.ascontiguousarray(c["z"], dtype=np.float64)
    other = np.ascontiguousarray(z[::-1] * 0.5 + 3.0)                      # the same shape, other data
    seg_start = a[3]
    K, sizes = int(seg_start[-1]), np.diff(seg_start)
    ctx = _lib.Context(0)
    try:
        for R in sx.LEVELS:
            ctx.profile(0)
            rows, tab, curve = ctx.fit_segments_refine(*a, R, cell_table=True, curve=True, z=z)
            n0 = ctx.profile_get()["k_profile"][0]
            assert n0 == 1 + launches_of(R, True)                         # the table and one chunk
            ctx.profile(0)
            ctx.fit_segments_refine(*a, R, cell_table=True, curve=True, z=other)
            assert ctx.profile_get()["k_profile"][0] == n0
            for n in (1, 7, K - 1, K, K + 1):
                # whole segments: a chunk takes the next segment while it stays within n cells
                chunks, s = 0, 0
                while s < len(sizes):
                    m = sizes[s]
                    s += 1
                    while s < len(sizes) and m + sizes[s] <= n:
                        m += sizes[s]
                        s += 1
                    chunks += 1
                ctx.set_option("fit_chunk", n)
                try:
                    ctx.profile(0)
                    got, gtab, gcurve = ctx.fit_segments_refine(*a, R, cell_table=True, curve=True, z=z)
                    launches = ctx.profile_get()["k_profile"][0]
                finally:
                    ctx.set_option("fit_chunk", 0)
                assert got.tobytes() == rows.tobytes() and gtab.tobytes() == tab.tobytes(), (R, n)
                assert gcurve.tobytes() == curve.tobytes(), (R, n)
                assert launches == 1 + chunks * launches_of(R, True), (R, n, launches, chunks)
    finally:
        ctx.close()


def test_matcher_route_gives_the_same_bytes_and_leaves_the_search_alone():
    g = synthetic.synthetic_scarp(768, theta=0.6)
    m = sl.Matcher(g)
    m.search(sl.Scarp, 100., _plan.age_grid()[::5], _plan.angle_grid())
    before = np.array(m.result_array())
    lo, hi = np.percentile(before[3][before[3] > 0], [60, 90])
    tr0 = m.extract_traces(lo, hi, 4)
    cells = np.flatnonzero(tr0.labels.ravel() > 0)
    lab = tr0.labels.ravel()[cells]
    assert len(cells) > 50
    for strike in ("cell", "segment"):
        a = m.fit_segments(tr0, 60., 3., return_cells=True, return_curve=True, strike=strike, refine=2)
        angle = before[2].ravel()[cells] if strike == "cell" else np.asarray(tr0.segments["strike"], dtype=np.float64)[lab - 1]
        b = sl.fit_segments(g, cells, lab, angle, 60., 3., return_cells=True, return_curve=True, refine=2)
        assert all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b)), strike
        assert a[0].dtype.names == SHARED + FINE and (a[0]["status"] != 1).sum() > 0
        plain = m.fit_segments(tr0, 60., 3., return_cells=True, return_curve=True, strike=strike)
        assert all(a[0][f].tobytes() == plain[0][f].tobytes() for f in SHARED) and a[2].tobytes() == plain[2].tobytes()
    # the search's record, its planes and the traces are what they were
    assert np.array_equal(np.array(m.result_array()), before, equal_nan=True)
    tr1 = m.extract_traces(lo, hi, 4)
    assert np.array_equal(tr0.labels, tr1.labels) and tr0.segments.tobytes() == tr1.segments.tobytes()


def test_library_refuses_what_the_header_says():
    import profile_reference as pr
    ctx = _lib.Context(0)
    z = pr.synthetic_z(64)
    ages = np.array([1.0, 2.0])
    one = (np.array([5 * 64 + 30], dtype=np.int64), np.array([0.0]), np.array([1.0]), np.array([0, 1], dtype=np.int64),
           np.array([1], dtype=np.int32))

    def fit(R=1, kt=ages, h=10, ms=4, mp=1, zz=z):
        return ctx.fit_segments_refine(*one, kt, h, 1, 1.0, 1.0, ms, mp, R, z=zz)
    try:
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-3\)"):
            ctx.fit_segments_refine(*one, ages, 10, 1, 1.0, 1.0, 4, 1, 1)  # no DEM set
        for R in (0, 1, 2):
            fit(R)
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-1\)"):
            fit(-1)
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\)"):
            fit(3)
        # what the plain call refuses, through the same checks
        for kw in (dict(kt=np.array([2.0, 1.0])), dict(ms=1), dict(mp=0)):
            with pytest.raises(_lib.ScarpletHipError, match=r"\(-1\)"):
                fit(**kw)
        for kw in (dict(kt=np.arange(1.0, 66.0)), dict(h=1025)):
            with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\)"):
                fit(**kw)
    finally:
        ctx.close()


def test_recovery_on_the_device():
    """The recovery case of tests/test_segment_refine_host.py, the 100 cells as ONE segment, R = 2: at noise 0 and 0.05 the
    device against the restatement by the rule above; at all three noise levels |kt_fine / kt0 - 1| is below a third of the
    grid's |kt / kt0 - 1| (noise 0.5 decides its last level inside 1e-8: held to the accuracy bound alone)."""
    for sigma in sx.SIGMAS:
        case = sx.recovery_case(sigma)
        table, cells = run_case(case, 2, return_curve=False)
        grid_off, fine_off = sx.recovery_figures(table[0])
        print("sigma %g: grid off by %.4g, fine off by %.4g, ratio %.3g" % (sigma, grid_off, fine_off, fine_off / grid_off))
        if sigma != 0.5:
            ref = sx.restate(case, 2)
            print(sx.compare(ref, sx.device_rows(table, by_position(case, cells), ref), case, 2))
        assert fine_off < grid_off / 3.0, (sigma, grid_off, fine_off)
