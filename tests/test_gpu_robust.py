"""Weights and robust fits of sl.fit_profiles on the MI355X (sc_fit_profiles_robust / _dem, docs/profiles.md) against the
numpy restatement (tests/robust_reference.py).

Every case runs through both routes - the DEM the matcher holds and the uploaded one - which must return the same bytes.

Tolerances and where they come from.  The anchors are exact: a product by 1 or by 2 is exact, so a plane of ones, a plane
of twos and a Huber constant no residual reaches must give the bits of the plain call.  Against the restatement the
tolerance is the profile family's (profile_reference.RTOL = 1e-9, scaled as its compare_rows scales): every compared fit
has a weighted, column-scaled design matrix of condition number <= COND_MAX = 1e3 (asserted on the restatement), and the
two CPU restatements (float64 lstsq, longdouble Gram-Schmidt; tests/test_robust_host.py) agree a hundred times closer on
these very inputs - the reweighting does not amplify rounding.  n, n_down and the status are equal; the indices are equal
except where the restatement's own value at the device's index is within RTOL of the one that decided (at most
TIE_SHARE = 1 % of a case's cells).
"""
import numpy as np
import pytest

import profile_reference as pr
import robust_reference as rr
import scarplet_amd as sl
from scarplet_amd import _lib

pytestmark = pytest.mark.gpu

LOSSES = ("huber", "tukey")
NAMES = ["pit surface", "carrizo h50 w2", "one age", "64 ages", "h31", "h32", "h15", "borders and corners", "NaN cells",
         "K = 0", "K = 1", "K = 5", "robust_scale given", "weights: a strip of zeros", "weights: random positive",
         "weights: NaN cells", "weights alone"]
CASES, REFS = {}, {}


def cases(loss):
    if loss not in CASES:
        CASES[loss] = rr.gpu_cases(loss)
    return CASES[loss]


def reference(loss, name):
    """The restatement's rows of a case: computed once, shared, left unchanged."""
    if (loss, name) not in REFS:
        REFS[(loss, name)] = rr.restate(cases(loss)[name])
    return REFS[(loss, name)]


def grid(z, de):
    return sl.DEMGrid.from_array(z, float(de))


def matcher(z, de):
    """The route without an upload (the matchers of a device share its context: the last one's DEM is the one it holds)."""
    return sl.Matcher(grid(z, de))


def run(z, de, cells, angle, h, w, **kw):
    """(table, curve) through both routes, which must agree in every byte."""
    a = sl.fit_profiles(grid(z, de), cells, angle, h * de, w * de, return_curve=True, **kw)
    b = matcher(z, de).fit_profiles(cells, h * de, w * de, angle=angle, return_curve=True, **kw)
    assert a[0].dtype == b[0].dtype and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    return a


def run_case(c, cells=None, angle=None):
    cells = c["cells"] if cells is None else cells
    angle = c["angle"] if angle is None else angle
    return run(c["z"], c["de"], cells, angle, c["h"], c["w"], ages=c["ages"], delta=c["delta"], min_samples=c["min_samples"],
               weights=c["weights"], **c["robust"])


def rows_of(table, curve):
    return [dict({f: table[f][k] for f in table.dtype.names}, curve=curve[k]) for k in range(len(table))]


def test_the_case_lists_are_the_ones_named_here():
    assert list(cases("huber")) == NAMES
    assert list(cases("tukey")) == NAMES[:13] + ["no age survives"] + NAMES[13:]


# ---- the anchors: bit for bit ----------------------------------------------------------------------------------------------
SHARED = [f for f in sl.profiles.FIT_DTYPE.names]


@pytest.mark.parametrize("name", ["pit surface", "NaN cells"])
def test_anchors_are_exact(name):
    c = cases("huber")[name]
    kw = dict(ages=c["ages"], delta=c["delta"], min_samples=c["min_samples"])
    args = (c["z"], c["de"], c["cells"], c["angle"], c["h"], c["w"])
    plain, pcurve = sl.fit_profiles(grid(c["z"], c["de"]), c["cells"], c["angle"], c["h"] * c["de"], c["w"] * c["de"],
                                    return_curve=True, **kw)
    fit = plain["status"] != 1
    assert fit.sum() >= 50
    ones, ocurve = run(*args, weights=np.ones(c["z"].shape), **kw)
    assert ones.dtype == sl.profiles.ROBUST_FIT_DTYPE
    for f in SHARED:
        assert ones[f].tobytes() == plain[f].tobytes(), f
    assert ocurve.tobytes() == pcurve.tobytes()
    assert ones["loss"].tobytes() == ones["sse"].tobytes() and np.isnan(ones["scale"]).all() and (ones["n_down"] == 0).all()
    assert np.array_equal(ones["ls_index"], ones["kt_index"])
    twos, tcurve = run(*args, weights=2.0 * np.ones(c["z"].shape), **kw)
    for f in ("cell", "n", "kt_index", "lo_index", "hi_index", "status", "kt", "kt_lo", "kt_hi", "a", "b", "c0"):
        assert twos[f].tobytes() == plain[f].tobytes(), f
    assert np.array_equal(twos["sse"][fit], 2.0 * plain["sse"][fit]) and np.array_equal(tcurve[fit], 2.0 * pcurve[fit])
    # a Huber constant no residual reaches: every factor is 1 in every iterate
    for w8 in (None, np.ones(c["z"].shape)):
        far, fcurve = run(*args, weights=w8, robust="huber", tuning=1e6, **kw)
        for f in SHARED + ["loss", "n_down", "ls_index"]:
            assert far[f].tobytes() == ones[f].tobytes(), f
        assert fcurve.tobytes() == ocurve.tobytes()
        assert far["loss"].tobytes() == far["sse"].tobytes() and (far["n_down"] == 0).all()
        assert np.array_equal(far["ls_index"], far["kt_index"]) and (far["scale"][fit] > 0).all()


# ---- against the restatement ---------------------------------------------------------------------------------------------------
ALL = [(loss, name) for loss in LOSSES for name in NAMES] + [("tukey", "no age survives")]


@pytest.mark.parametrize("loss,name", ALL)
def test_against_the_restatement(loss, name):
    c = cases(loss)[name]
    table, curve = run_case(c)
    K, A = len(c["cells"]), len(c["ages"])
    assert table.dtype == sl.profiles.ROBUST_FIT_DTYPE and len(table) == K and curve.shape == (K, A)
    nx = c["z"].shape[1]
    assert np.array_equal(table["cell"], c["cells"]) and np.array_equal(table["row"] * nx + table["col"], c["cells"])
    assert np.array_equal(table["height"], 2.0 * table["a"], equal_nan=True)
    st = rr.compare_rows(c, reference(loss, name), rows_of(table, curve))
    print("%s, %s: %s" % (loss, name, st))
    fit = (table["status"] & 1) == 0
    assert np.array_equal(table["rmse"][fit], np.sqrt(table["loss"][fit] / (table["n"][fit] - 3)))
    assert np.array_equal(table["kt"][fit], c["ages"][table["kt_index"][fit]])
    assert np.array_equal(table["kt_lo"][fit], c["ages"][table["lo_index"][fit]])
    assert np.array_equal(table["kt_hi"][fit], c["ages"][table["hi_index"][fit]])
    assert np.array_equal(curve[fit, table["kt_index"][fit]], table["loss"][fit])
    assert np.isnan(curve[~fit]).all()
    if name == "no age survives":
        assert (table["status"] == 33).all() and (table["scale"] == 1e-9).all()
    if name in ("h31", "h32", "h15", "weights: random positive"):
        if loss == "tukey":
            assert np.isnan(curve[fit]).any()                              # ages that lost their support, beside ones that won
    missing = int((fit & (table["n"] < 2 * c["h"] + 1)).sum())              # fitted with points missing
    if name in ("borders and corners", "NaN cells", "weights: a strip of zeros"):
        assert missing >= 20
    if name == "weights: NaN cells":
        assert missing >= 2


# ---- no scale ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", LOSSES)
def test_zero_scale_returns_the_least_squares_row(loss):
    """A noise-free plane.  The slope is 2^-6, not 0.01, and the profiles run along the rows: 0.01 x is no plane in
    float64 - its samples carry rounding of 1e-16, the residuals of the fit are that rounding (the restatement's median
    |r| on z = 0.01 x is 6e-17 at angle 0 and 1e-16 at angle 0.3, not 0) and nothing about them can be compared.  With a
    dyadic slope every sample, mean and sum is exact, the residuals are 0 and so is sigma."""
    n = 96
    z = 0.015625 * np.arange(n, dtype=np.float64)[None, :] * np.ones((n, 1))
    cells = np.array([48 * n + 48, 40 * n + 50, 30 * n + 10])
    kw = dict(ages=[1.0, 10.0, 100.0], min_samples=4)
    plain = sl.fit_profiles(grid(z, 1.0), cells, 0.0, 20.0, 1.0, **kw)
    got, curve = run(z, 1.0, cells, 0.0, 20, 1, robust=loss, **kw)
    assert (got["scale"] == 0.0).all() and (got["status"] & 16 == 16).all() and (got["n_down"] == 0).all()
    for f in SHARED:
        if f != "status":
            assert got[f].tobytes() == plain[f].tobytes(), f
    assert np.array_equal(got["status"], plain["status"] | 16)
    assert got["loss"].tobytes() == got["sse"].tobytes() and np.array_equal(got["ls_index"], got["kt_index"])
    # (the longdouble twin: on these inputs Gram-Schmidt is exact as the device's is, LAPACK's lstsq is not)
    ref = rr.fit_profiles(z, None, 1.0, cells, 0.0, 20, 1, np.array(kw["ages"]), robust=loss, fit=rr.wfit_longdouble)
    assert [r["status"] for r in ref] == got["status"].tolist() and all(r["scale"] == 0.0 for r in ref)
    assert [r["kt_index"] for r in ref] == got["kt_index"].tolist() and all(r["sse"] == 0.0 for r in ref)


# ---- determinism ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", LOSSES)
def test_two_runs_and_a_permutation_return_the_same_rows(loss):
    c = cases(loss)["weights: NaN cells"]
    table, curve = run_case(c)
    again, acurve = run_case(c)
    assert again.tobytes() == table.tobytes() and acurve.tobytes() == curve.tobytes()
    perm = np.random.default_rng(3).permutation(len(c["cells"]))
    ptable, pcurve = run_case(c, c["cells"][perm], c["angle"][perm])
    assert ptable.tobytes() == table[perm].tobytes() and pcurve.tobytes() == curve[perm].tobytes()
    only = sl.fit_profiles(grid(c["z"], c["de"]), c["cells"], c["angle"], c["h"] * c["de"], c["w"] * c["de"], ages=c["ages"],
                           delta=c["delta"], min_samples=c["min_samples"], weights=c["weights"], **c["robust"])
    assert only.tobytes() == table.tobytes()                               # the run without the curve


# ---- what the feature is for ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", LOSSES)
def test_the_pit_surface_shares(loss):
    """The device's share of cells on the true age index is the restatement's, less one cell at the most."""
    c = cases(loss)["pit surface"]
    table, _ = run_case(c)
    want = rr.share_on(reference(loss, "pit surface"))
    got = int((table["kt_index"] == rr.PIT_TRUE_INDEX).sum())
    plain = int((table["ls_index"] == rr.PIT_TRUE_INDEX).sum())
    print("%s: %d of %d cells on the true index (restatement %d; least squares %d)" % (loss, got, len(table), want, plain))
    assert got >= want - 1


def test_matcher_route_takes_traces_and_adds_the_label():
    c = cases("huber")["pit surface"]
    m = matcher(c["z"], c["de"])
    from scarplet_amd import traces
    labels = np.zeros(c["z"].shape, dtype=np.int32)
    labels.ravel()[c["cells"]] = 7
    tr = traces.Traces(labels > 0, labels, traces._table(np.zeros(0, dtype=_lib.SEGMENT_DTYPE)))
    cells = np.flatnonzero(labels.ravel() > 0)
    a = m.fit_profiles(tr, 100.0, 2.0, min_samples=15, angle=0.2, robust="tukey")
    b = sl.fit_profiles(grid(c["z"], c["de"]), cells, 0.2, 100.0, 2.0, min_samples=15, robust="tukey")
    assert a.dtype.names == b.dtype.names + ("label",) and (a["label"] == 7).all()
    for f in b.dtype.names:
        assert a[f].tobytes() == b[f].tobytes(), f


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_library_refuses_what_the_header_says(gpu_ctx):
    ctx = _lib.Context(0)
    z = pr.synthetic_z(64)
    ages = np.array([1.0, 2.0])
    one = (np.array([5 * 64 + 30], dtype=np.int64), np.array([0.0]), np.array([1.0]))

    def fit(kt=ages, h=10, w=1, ms=4, zz=z, **kw):
        args = dict(loss=_lib.ROBUST_HUBER, tuning=1.345, iterations=8, scale=0.0)
        args.update(kw)
        return ctx.fit_profiles_robust(*one, kt, h, w, 1.0, 1.0, ms, z=zz, **args)
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-3\)"):
        ctx.fit_profiles_robust(*one, ages, 10, 1, 1.0, 1.0, 4, loss=_lib.ROBUST_HUBER, tuning=1.0, iterations=1)     # no DEM set
    rows, _ = fit()
    assert rows["status"][0] & 1 == 0
    fit(iterations=64)
    fit(loss=_lib.ROBUST_NONE, tuning=0.0, iterations=0)                   # without a loss its arguments are not read
    for kw in (dict(loss=3), dict(loss=-1), dict(tuning=0.0), dict(tuning=np.nan), dict(tuning=np.inf), dict(iterations=0),
               dict(scale=-1.0), dict(scale=np.nan), dict(ms=1), dict(kt=np.array([2.0, 1.0]))):
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-1\)"):
            fit(**kw)
    for kw in (dict(iterations=65), dict(kt=np.arange(1.0, 66.0)), dict(h=1025), dict(w=33)):
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\)"):
            fit(**kw)
    ctx.close()
