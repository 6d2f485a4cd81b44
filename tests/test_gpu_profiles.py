"""sl.fit_profiles on the MI355X (sc_fit_profiles / sc_fit_profiles_dem, docs/profiles.md) against the numpy
restatement (tests/profile_reference.py).

Tolerances and where they come from.  Every compared fit has a column-scaled design matrix of condition number
<= 1e3 (a condition on the inputs, asserted on the restatement).  Under that cap even a solver that squared the
condition number would stay near 1e6 x 1.1e-16 = 1e-10, and the two CPU restatements (float64 lstsq, longdouble
Gram-Schmidt; tests/test_profile_host.py) agree to 6e-13 in sse and 9e-11 of the range in the coefficients on these
very inputs.  So: sse within 1e-9 relative; c0, b h de and a within 1e-9 of the profile's peak-to-peak range; n and
status equal; kt_index, lo_index and hi_index equal except where the restatement's own sse at the device's index is
within 1e-9 relative of the value that decided - such cells are counted and may be at most 1 % of a case.
"""
import numpy as np
import pytest

import profile_reference as pr
import scarplet_amd as sl
from scarplet_amd import _lib, _plan, synthetic

pytestmark = pytest.mark.gpu


def grid(z, de):
    return sl.DEMGrid.from_array(z, float(de))


def rows_of(table, curve, idx):
    return [dict({f: table[f][k] for f in table.dtype.names}, curve=None if curve is None else curve[k]) for k in idx]


def run_case(case, return_curve=True):
    h, w, de = case["h"], case["w"], case["de"]
    return sl.fit_profiles(grid(case["z"], de), case["cells"], case["angle"], h * de, w * de, ages=case["ages"],
                           delta=case["delta"], min_samples=case["min_samples"], return_curve=return_curve)


CASES = None


def cases():
    global CASES
    if CASES is None:
        CASES = pr.gpu_cases()
    return CASES


NAMES = ["carrizo h50 w2", "carrizo h50 w0", "grandcanyon h100 w5", "synthetic h100 w0", "synthetic h100 w5",
         "synthetic h30 w5", "synthetic h15 w2", "multiples of pi/4", "repeated cells", "one age", "64 ages", "h2",
         "one cell", "no cell", "borders and corners", "NaN cells", "h1024", "a million cells"]


def test_the_case_list_is_the_one_named_here():
    assert [c["name"] for c in cases()] == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_against_the_restatement(name):
    case = cases()[NAMES.index(name)]
    table, curve = run_case(case)
    K, A = len(case["cells"]), len(case["ages"])
    assert table.dtype.names[:3] == ("row", "col", "cell") and len(table) == K and curve.shape == (K, A)
    nx = case["z"].shape[1]
    assert np.array_equal(table["cell"], case["cells"])                    # input order, repeats included
    assert np.array_equal(table["row"] * nx + table["col"], case["cells"])
    assert np.array_equal(table["height"], 2.0 * table["a"], equal_nan=True)
    idx, ref = pr.restate(case)
    st = pr.compare_rows(ref, rows_of(table, curve, idx), case["h"], case["de"], case["delta"])
    print("%s: %s" % (name, st))
    fit = table["status"] != 1
    assert np.array_equal(table["rmse"][fit], np.sqrt(table["sse"][fit] / (table["n"][fit] - 3)))
    assert np.array_equal(table["kt"][fit], case["ages"][table["kt_index"][fit]])
    assert np.array_equal(table["kt_lo"][fit], case["ages"][table["lo_index"][fit]])
    assert np.array_equal(table["kt_hi"][fit], case["ages"][table["hi_index"][fit]])
    assert np.array_equal(curve[fit, table["kt_index"][fit]], table["sse"][fit])
    assert np.isnan(curve[~fit]).all()
    if name in ("borders and corners", "NaN cells"):
        n = np.array([r["n"] for r in ref])
        s = np.array([r["status"] for r in ref])
        assert (s == 1).sum() > 0 or name == "NaN cells"
        assert ((s != 1) & (n < 2 * case["h"] + 1)).sum() >= 20            # fitted with points missing
    if name == "repeated cells":
        for k in range(0, K, 3):
            assert table[k:k + 3].tobytes() == table[k:k + 1].tobytes() * 3
    # a second run and the run without the curve: the same bytes
    again = run_case(case, return_curve=False)
    assert again.tobytes() == table.tobytes()


def test_matcher_route_gives_the_same_bytes_and_leaves_the_search_alone():
    g = synthetic.synthetic_scarp(768, theta=0.6)
    m = sl.Matcher(g)
    m.search(sl.Scarp, 100., _plan.age_grid()[::5], _plan.angle_grid())
    before = np.array(m.result_array())
    lo, hi = np.percentile(before[3][before[3] > 0], [60, 90])
    tr0 = m.extract_traces(lo, hi, 4)
    cells = np.flatnonzero(tr0.labels.ravel() > 0)
    assert len(cells) > 50
    a = m.fit_profiles(tr0, 60., 3.)
    assert a.dtype.names[-1] == "label" and np.array_equal(a["label"], tr0.labels.ravel()[cells])
    assert np.array_equal(a["cell"], cells)
    b = m.fit_profiles(cells, 60., 3.)                                     # the cells by hand: the angle plane is read
    c, curve = sl.fit_profiles(g, cells, before[2], 60., 3., return_curve=True)      # the upload route
    d = sl.fit_profiles(g, tr0.labels > 0, before[2].ravel()[cells], 60., 3.)
    from numpy.lib import recfunctions
    without_label = recfunctions.repack_fields(a[list(c.dtype.names)])     # (the label column packs last)
    assert without_label.dtype == c.dtype
    assert without_label.tobytes() == b.tobytes() == c.tobytes() == d.tobytes()
    assert (c["status"] != 1).sum() > 50
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
    one = (np.array([5], dtype=np.int64), np.array([0.0]), np.array([1.0]))

    def fit(cells=one[0], sa=one[1], ca=one[2], kt=ages, h=10, w=1, de=1.0, delta=1.0, ms=4, zz=z):
        return ctx.fit_profiles(cells, sa, ca, kt, h, w, de, delta, ms, z=zz)
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-3\)"):
        ctx.fit_profiles(*one, ages, 10, 1, 1.0, 1.0, 4)                   # no DEM set
    fit()
    for kw in (dict(cells=np.array([64 * 64], dtype=np.int64)), dict(sa=np.array([np.nan])), dict(kt=np.array([2.0, 1.0])),
               dict(kt=np.array([0.0, 1.0])), dict(ms=1), dict(ms=11), dict(delta=-1.0), dict(delta=np.inf),
               dict(zz=z[:1].copy()), dict(de=0.0)):
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-1\)"):
            fit(**kw)
    for kw in (dict(kt=np.arange(1.0, 66.0)), dict(h=1025, ms=4), dict(w=33)):
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\)"):
            fit(**kw)
    # a context that holds a block of a larger grid
    zb = np.ascontiguousarray(z[:40, :])
    ax = np.arange(64.0)
    ctx.set_dem(zb, 1.0, 1.0, ax, ax, origin=(0, 0), shape=(64, 64), core=(0, 32, 0, 64), wrap=False)
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\)"):
        ctx.fit_profiles(*one, ages, 10, 1, 1.0, 1.0, 4)
    ctx.close()


# The CPU pair this test's thresholds come from (docs/profiles.md, "Against the search"): the oracle's search
# restricted to +-0.3 rad around the scarp on synthetic_scarp(256) and the restatement on its thinned cells gave
# SIGN_SHARE of agreeing signs and a median index difference of INDEX_MEDIAN grid steps (33 cells, the largest
# difference 8).  The share is 0, not 1: the search forms ifft(fft(curv) fft(W)), a convolution, and the Scarp window is
# odd, so its amp is MINUS the offset a scarp's erf carries along the profile (amp -1.45 where a = +1.00).  The two
# signs are opposite in every cell, which pins the direction just as well - OPPOSITE_SHARE is what is asked for, next
# to the share itself.
SIGN_SHARE = 0.0
OPPOSITE_SHARE = 1.0
INDEX_MEDIAN = 2.0


def test_end_to_end_agrees_with_the_search():
    """sl.match -> extract_traces -> Matcher.fit_profiles on the largest segment of synthetic_scarp(1024): the sign
    of the fitted a against the sign of amp, the fitted age index against the search's.  With the step of the profile
    reversed every sign flips."""
    g = synthetic.synthetic_scarp(1024)
    m = sl.Matcher(g)
    res = np.array(m.search(sl.Scarp, 100., _plan.age_grid(), _plan.angle_grid()).result_array())
    smax = np.nanmax(res[3])
    tr = m.extract_traces(0.2 * smax, 0.5 * smax, 50)
    k = int(np.argmax(tr.segments["n_cells"]))
    fits = m.fit_profiles(tr, 100.)
    fits = fits[(fits["label"] == tr.segments["label"][k]) & (fits["status"] != 1)]
    assert len(fits) > 100
    amp, age = res[0].ravel()[fits["cell"]], res[1].ravel()[fits["cell"]]
    share = np.mean(np.sign(fits["a"]) == np.sign(amp))
    ages = _plan.age_grid()
    search_index = np.array([int(np.argmin(np.abs(ages - v))) for v in age])
    diff = np.median(np.abs(fits["kt_index"] - search_index))
    print("largest segment: %d fitted cells, %.4f of the signs agree, median |index difference| %g" % (len(fits), share, diff))
    assert share >= SIGN_SHARE - 0.01
    assert np.mean(np.sign(fits["a"]) == -np.sign(amp)) >= OPPOSITE_SHARE - 0.01
    assert diff <= INDEX_MEDIAN + 1
