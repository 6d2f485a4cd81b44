"""sl.fit_profiles(refine=R) on the MI355X (sc_fit_profiles_refine / sc_fit_profiles_refine_dem; docs/profiles.md,
"Continuous ages") against the numpy restatement (tests/refine_reference.py).

What is compared, and where the tolerances come from.
* The shared fields and the curves are the plain call's bytes: no tolerance.
* sse_fine is within 1e-9 relative of the restatement's own float64 lstsq sse at the device's kt_fine, unconditionally, and
  a_fine, b_fine h de and c0_fine are within 1e-9 of the profile's range of that fit: the tolerances of
  tests/test_gpu_profiles.py, derived in its header, on the same condition - every compared design matrix, the candidates'
  included, has a column-scaled condition number <= 1e3, asserted on the restatement.
* kt_fine, kt_lo_fine, kt_hi_fine and status_fine are bit-equal to the restatement's, except where the decision that parted
  was taken inside 1e-9 relative.  The restatement keeps, for the minimum and for either end, the margin of the closest
  decision on its way: at every level the distance of the runner-up (a candidate of another age) from the pick, and of the
  last pick from the grid's best, for the minimum; the distance of every grid sse of the walk and of every candidate from
  thr, for an end.  A pick that differs must find that margin <= 1e-9; such cells are counted and may be at most 1 % of a
  case (a cell whose minimum parted is counted once, and its ends - which follow the minimum - are not looked at).  On these
  inputs float64 lstsq and longdouble Gram-Schmidt part in no cell (tests/test_refine_host.py).
"""
import numpy as np
import pytest

import refine_reference as rf
import scarplet_amd as sl
from scarplet_amd import _lib, _plan, synthetic

pytestmark = pytest.mark.gpu

SHARED = ("row", "col", "cell", "n", "kt_index", "lo_index", "hi_index", "status", "kt", "kt_lo", "kt_hi", "a", "b", "c0", "sse",
          "rmse", "height")
GRID_OF = dict(kt_fine="kt", kt_lo_fine="kt_lo", kt_hi_fine="kt_hi", a_fine="a", b_fine="b", c0_fine="c0", sse_fine="sse",
               rmse_fine="rmse", height_fine="height", status_fine="status")


def grid(z, de):
    return sl.DEMGrid.from_array(z, float(de))


def run_case(case, refine, return_curve=True):
    h, w, de = case["h"], case["w"], case["de"]
    return sl.fit_profiles(grid(case["z"], de), case["cells"], case["angle"], h * de, w * de, ages=case["ages"],
                           delta=case["delta"], min_samples=case["min_samples"], return_curve=return_curve, refine=refine)


def rows_of(table):
    return [{f: table[f][k] for f in table.dtype.names} for k in range(len(table))]


def test_the_case_list_is_the_one_named_here():
    assert [c["name"] for c in rf.gpu_cases()] == rf.NAMES == [
        "synthetic h100 w2", "synthetic h15 w0", "h2", "one age", "64 ages", "best age below the grid", "best age above the grid",
        "borders, corners and NaN cells", "repeated cells", "no cell", "h1024"]


@pytest.mark.parametrize("R", rf.LEVELS)
@pytest.mark.parametrize("name", rf.NAMES)
def test_against_the_restatement(name, R):
    case = rf.gpu_cases()[rf.NAMES.index(name)]
    K, A = len(case["cells"]), len(case["ages"])
    table, curve = run_case(case, R)
    assert table.dtype.names == SHARED + rf.FINE_FLOATS + ("status_fine",) and len(table) == K and curve.shape == (K, A)
    # the shared fields and the curves: the plain call's bytes
    plain, pcurve = run_case(case, None)
    assert plain.dtype.names == SHARED
    for f in SHARED:
        assert table[f].tobytes() == plain[f].tobytes(), f
    assert curve.tobytes() == pcurve.tobytes()
    # no level: every fine field is its grid counterpart
    zero, zcurve = run_case(case, 0)
    assert zero.dtype == table.dtype and zcurve.tobytes() == pcurve.tobytes()
    for f, g in GRID_OF.items():
        assert zero[f].tobytes() == plain[g].astype(zero[f].dtype).tobytes(), f
    # the restatement
    st = rf.compare(rf.reference(name, R), rows_of(table), case, R)
    print("%s, R = %d: %s" % (name, R, st))
    # structure (per cell in compare; here what concerns the table as a whole)
    fit = table["status"] != 1
    assert np.all(table["sse_fine"][fit] <= table["sse"][fit])
    assert np.all((table["kt_lo_fine"][fit] <= table["kt_fine"][fit]) & (table["kt_fine"][fit] <= table["kt_hi_fine"][fit]))
    assert np.array_equal(table["rmse_fine"][fit], np.sqrt(table["sse_fine"][fit] / (table["n"][fit] - 3)))
    assert np.array_equal(table["height_fine"], 2.0 * table["a_fine"], equal_nan=True)
    assert np.all(table["status_fine"][~fit] == 1) and np.all((table["status_fine"][fit] & ~6) == 0)
    for f in rf.FINE_FLOATS:
        assert np.isnan(table[f][~fit]).all() and not np.isnan(table[f][fit]).any(), f
    # a fine age that is a grid age - the grid's best kept, or a candidate at a bracket's end - has the grid fit's bits: the
    # candidate's column is the table's, and its sums run in the grid fit's order
    on = fit & (table["kt_fine"] == table["kt"])
    for f, g in (("sse_fine", "sse"), ("a_fine", "a"), ("b_fine", "b"), ("c0_fine", "c0")):
        assert table[f][on].tobytes() == table[g][on].tobytes(), f
    if name == "borders, corners and NaN cells":
        assert (~fit).sum() > 0 and (fit & (table["n"] < 2 * case["h"] + 1)).sum() >= 5
    if name == "best age below the grid":
        assert ((table["kt_index"] == 0) & (table["status_fine"] & 2 > 0)).sum() > K // 2
    if name == "best age above the grid":
        assert ((table["kt_index"] == A - 1) & (table["status_fine"] & 4 > 0)).sum() > K // 2
    if name in ("one age", "h2"):
        assert np.all(table["kt_fine"][fit] == case["ages"][0]) and np.all(table["status_fine"][fit] == 6)
    if name == "repeated cells":
        for k in range(0, K, 3):
            assert table[k:k + 3].tobytes() == table[k:k + 1].tobytes() * 3
    # a second run and the run without the curve: the same bytes
    assert run_case(case, R)[0].tobytes() == table.tobytes()
    assert run_case(case, R, return_curve=False).tobytes() == table.tobytes()


def test_in_many_chunks_the_same_bytes():
    """The option "fit_chunk" bounds this call's chunks as it does every per-cell call's: on a context of its own, through the
    binding (the raw rows, padding included), on an uploaded DEM."""
    from scarplet_amd import profiles
    c = rf.gpu_cases()[rf.NAMES.index("borders, corners and NaN cells")]
    a = profiles.check_args(c["z"].shape, c["de"], c["cells"], c["angle"], c["h"] * c["de"], c["w"] * c["de"], c["ages"],
                            c["delta"], c["min_samples"])
    z = np.ascontiguousarray(c["z"], dtype=np.float64)
    K = len(a[0])
    ctx = _lib.Context(0)
    try:
        for R in rf.LEVELS:
            ctx.profile(0)
            rows, curve = ctx.fit_profiles_refine(*a, R, curve=True, z=z)
            n0 = ctx.profile_get()["k_profile"][0]
            assert n0 == 2                                                # the table and one launch
            for n in (1, 7, K - 1, K, K + 1):
                ctx.set_option("fit_chunk", n)
                try:
                    ctx.profile(0)
                    got, gcurve = ctx.fit_profiles_refine(*a, R, curve=True, z=z)
                    launches = ctx.profile_get()["k_profile"][0]
                finally:
                    ctx.set_option("fit_chunk", 0)
                assert got.tobytes() == rows.tobytes() and gcurve.tobytes() == curve.tobytes(), (R, n)
                assert launches - n0 == -(-K // n) - 1, (R, n, launches)
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
    assert len(cells) > 50
    a = m.fit_profiles(tr0, 60., 3., refine=2)
    assert a.dtype.names[-1] == "label" and np.array_equal(a["label"], tr0.labels.ravel()[cells])
    assert np.array_equal(a["cell"], cells)
    b = m.fit_profiles(cells, 60., 3., refine=2)                           # the cells by hand: the angle plane is read
    c, curve = sl.fit_profiles(g, cells, before[2], 60., 3., return_curve=True, refine=2)      # the upload route
    from numpy.lib import recfunctions
    without_label = recfunctions.repack_fields(a[list(c.dtype.names)])     # (the label column packs last)
    assert without_label.dtype == c.dtype
    assert without_label.tobytes() == b.tobytes() == c.tobytes()
    assert (c["status"] != 1).sum() > 50 and (c["kt_fine"] != c["kt"]).sum() > 25
    plain, pcurve = m.fit_profiles(cells, 60., 3., return_curve=True)
    assert all(c[f].tobytes() == plain[f].tobytes() for f in plain.dtype.names) and curve.tobytes() == pcurve.tobytes()
    # the search's record, its planes and the traces are what they were
    assert np.array_equal(np.array(m.result_array()), before, equal_nan=True)
    tr1 = m.extract_traces(lo, hi, 4)
    assert np.array_equal(tr0.labels, tr1.labels) and tr0.segments.tobytes() == tr1.segments.tobytes()


def test_library_refuses_what_the_header_says(gpu_ctx):
    import profile_reference as pr
    ctx = _lib.Context(0)
    z = pr.synthetic_z(64)
    ages = np.array([1.0, 2.0])
    one = (np.array([5], dtype=np.int64), np.array([0.0]), np.array([1.0]))

    def fit(R=1, kt=ages, h=10, ms=4, zz=z):
        return ctx.fit_profiles_refine(*one, kt, h, 1, 1.0, 1.0, ms, R, z=zz)
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-3\)"):
        ctx.fit_profiles_refine(*one, ages, 10, 1, 1.0, 1.0, 4, 1)        # no DEM set
    for R in (0, 1, 2):
        fit(R)
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-1\)"):
        fit(-1)
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\)"):
        fit(3)
    # what the plain call refuses, through the same checks
    for kw in (dict(kt=np.array([2.0, 1.0])), dict(ms=1), dict(ms=11), dict(zz=z[:1].copy())):
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-1\)"):
            fit(**kw)
    for kw in (dict(kt=np.arange(1.0, 66.0)), dict(h=1025)):
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\)"):
            fit(**kw)
    # a context that holds a block of a larger grid
    zb = np.ascontiguousarray(z[:40, :])
    ax = np.arange(64.0)
    ctx.set_dem(zb, 1.0, 1.0, ax, ax, origin=(0, 0), shape=(64, 64), core=(0, 32, 0, 64), wrap=False)
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\)"):
        ctx.fit_profiles_refine(*one, ages, 10, 1, 1.0, 1.0, 4, 1)
    ctx.close()


def test_recovery_on_the_device():
    """The recovery case of tests/test_refine_host.py at sigma = 0.05: the device's median |kt_fine / kt0 - 1| is at most the
    restatement's plus one step of the last level, 2 (ages[i + 1] - ages[i - 1]) / 63^2 at the grid age above kt0."""
    case = rf.recovery_case(0.05)
    ref = rf.recovery_figures(rf.restate(case, 2), case["ages"])
    table = run_case(case, 2, return_curve=False)
    dev = rf.recovery_figures(rows_of(table), case["ages"])
    i = int(np.searchsorted(case["ages"], rf.KT0))
    step = 2.0 * (case["ages"][i + 1] - case["ages"][i - 1]) / 63.0 ** 2 / rf.KT0
    print("device %s\nrestatement %s\nlast-level step %.3g" % (dev, ref, step))
    assert dev["fine_median"] <= ref["fine_median"] + step
    assert dev["fine_median"] < dev["grid_median"]
