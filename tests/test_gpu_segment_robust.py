"""Weights and robust fits of sl.fit_segments on the MI355X (sc_fit_segments_robust / _dem, docs/segments.md) against the
numpy restatement (tests/segment_robust_reference.py).

Tolerances and where they come from.  The anchors are exact: a product by 1 or by 2 is exact, so a plane of ones, a plane
of twos and a Huber constant no residual reaches must give the bits of the plain call, and a segment of one usable
profile runs the single-profile call's operations in its order.  Against the restatement the tolerance is the profile
family's (profile_reference.RTOL = 1e-9, scaled as segment_reference.compare and robust_reference.compare_rows scale):
every compared fit has a weighted, column-scaled design matrix of condition number <= COND_MAX = 1e3 (asserted on the
restatement), and the two CPU restatements (float64 lstsq on the full matrix, longdouble Frisch-Waugh;
tests/test_segment_robust_host.py) agree a hundred times closer on these very inputs.  The counts, n_down, n_dormant, the
per-cell flags and the status are equal; the indices are equal except where the restatement's own value at the device's
index is within RTOL of the one that decided.
"""
import numpy as np
import pytest

import profile_reference as pr
import segment_robust_reference as qr
import scarplet_amd as sl
from scarplet_amd import _lib, segments, traces

pytestmark = pytest.mark.gpu

LOSSES = ("huber", "tukey")
NAMES = ["sizes 1 2 63 64 65 129", "h31", "h32", "h15", "one age", "64 ages", "no cell", "labels <= 0 only", "not fitted",
         "borders", "NaN cells", "robust_scale given", "weights: a strip of zeros", "weights: random positive",
         "weights: NaN cells", "weights alone", "block"]
CASES, REFS = {}, {}


def cases(loss):
    if loss not in CASES:
        CASES[loss] = qr.gpu_cases(loss)
    return CASES[loss]


def reference(loss, name):
    """The restatement's rows of a case: computed once, shared, left unchanged."""
    if (loss, name) not in REFS:
        REFS[(loss, name)] = qr.restate(cases(loss)[name])
    return REFS[(loss, name)]


def grid(z, de):
    return sl.DEMGrid.from_array(z, float(de))


def run(z, de, cells, labels, angle, h, w, **kw):
    return sl.fit_segments(grid(z, de), cells, labels, angle, h * de, w * de, return_cells=True, return_curve=True, **kw)


def run_case(c, **over):
    kw = dict(ages=c["ages"], delta=c["delta"], min_samples=c["min_samples"], min_profiles=c["min_profiles"],
              weights=c["weights"], **c["robust"])
    kw.update(over)
    return run(c["z"], c["de"], c["cells"], c["labels"], c["angle"], c["h"], c["w"], **kw)


def by_position(ct, c):
    """The cell table (input order of the kept cells) indexed by input position."""
    full = np.zeros(len(c["cells"]), dtype=ct.dtype)
    full[np.flatnonzero(c["labels"] > 0)] = ct
    return full


def test_the_case_lists_are_the_ones_named_here():
    assert list(cases("huber")) == NAMES
    assert list(cases("tukey")) == NAMES[:12] + ["no age survives"] + NAMES[12:]


# ---- the anchors: bit for bit ----------------------------------------------------------------------------------------------
SHARED = list(segments.FIT_DTYPE.names)
SHARED_CELL = list(segments.CELL_DTYPE.names)


@pytest.mark.parametrize("name", ["sizes 1 2 63 64 65 129", "NaN cells", "not fitted"])
def test_anchors_are_exact(name):
    c = cases("huber")[name]
    kw = dict(ages=c["ages"], delta=c["delta"], min_samples=c["min_samples"], min_profiles=c["min_profiles"])
    args = (c["z"], c["de"], c["cells"], c["labels"], c["angle"], c["h"], c["w"])
    plain, pct, pcurve = run(*args, **kw)
    assert plain.dtype == segments.FIT_DTYPE and pct.dtype == segments.CELL_DTYPE
    fit = plain["status"] != 1
    assert fit.sum() >= 1
    # 1. a plane of ones alone: the plain call's bytes in every shared field of rows, cell table and curve
    ones, oct_, ocurve = run(*args, weights=np.ones(c["z"].shape), **kw)
    assert ones.dtype == segments.ROBUST_FIT_DTYPE and oct_.dtype == segments.ROBUST_CELL_DTYPE
    for f in SHARED:
        assert ones[f].tobytes() == plain[f].tobytes(), f
    for f in SHARED_CELL:
        assert oct_[f].tobytes() == pct[f].tobytes(), f
    assert ocurve.tobytes() == pcurve.tobytes()
    assert ones["loss"].tobytes() == ones["sse"].tobytes() and np.isnan(ones["scale"]).all()
    assert (ones["n_down"] == 0).all() and (ones["n_dormant"] == 0).all() and np.array_equal(ones["ls_index"], ones["kt_index"])
    assert oct_["loss"].tobytes() == oct_["sse"].tobytes() and (oct_["n_down"] == 0).all() and (oct_["dormant"] == 0).all()
    # 2. a plane of twos: the same indices and coefficients, exactly twice the sse
    twos, tct, tcurve = run(*args, weights=2.0 * np.ones(c["z"].shape), **kw)
    for f in ("label", "n_cells", "n_profiles", "n", "dof", "kt_index", "lo_index", "hi_index", "status", "kt", "kt_lo", "kt_hi", "a"):
        assert twos[f].tobytes() == plain[f].tobytes(), f
    for f in ("cell", "used", "n", "b", "c0"):
        assert tct[f].tobytes() == pct[f].tobytes(), f
    assert np.array_equal(twos["sse"][fit], 2.0 * plain["sse"][fit]) and np.array_equal(tcurve[fit], 2.0 * pcurve[fit])
    assert np.array_equal(tct["sse"], 2.0 * pct["sse"], equal_nan=True)
    # 3. a Huber constant no residual reaches: every factor is 1 in every iterate
    for w8 in (None, np.ones(c["z"].shape)):
        far, fct, fcurve = run(*args, weights=w8, robust="huber", tuning=1e6, **kw)
        for f in SHARED + ["loss", "n_down", "ls_index", "n_dormant"]:
            assert far[f].tobytes() == ones[f].tobytes(), f
        for f in SHARED_CELL + ["loss", "n_down", "dormant"]:
            assert fct[f].tobytes() == oct_[f].tobytes(), f
        assert fcurve.tobytes() == ocurve.tobytes()
        assert far["loss"].tobytes() == far["sse"].tobytes() and (far["n_down"] == 0).all() and (far["n_dormant"] == 0).all()
        assert np.array_equal(far["ls_index"], far["kt_index"]) and (far["scale"][fit] > 0).all()


ONE_FIELDS = ("kt_index", "lo_index", "hi_index", "status", "a", "sse", "rmse", "loss", "scale", "n_down", "ls_index", "kt",
              "kt_lo", "kt_hi", "height")


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name,extra", [("h31", {}), ("NaN cells", {}), ("weights: NaN cells", {}), ("weights: random positive", {}),
                                        ("robust_scale given", {}), ("h15", dict(robust=None, iterations=8))])
def test_one_profile_segments_are_fit_profiles_byte_for_byte(loss, name, extra):
    """4. A segment of ONE usable profile: the single-profile call's row, and its b and c0 in the cell table."""
    c = cases(loss)[name]
    K = len(c["cells"])
    lab = np.random.default_rng(3).permutation(K) + 1                      # one segment per cell, in shuffled order
    h, w, de = c["h"], c["w"], c["de"]
    kw = dict(ages=c["ages"], delta=c["delta"], min_samples=c["min_samples"], weights=c["weights"], **c["robust"])
    kw.update(extra)
    if kw["robust"] is None:
        kw["weights"] = np.full(c["z"].shape, 0.75)                        # weights alone
    seg, ct, cv = sl.fit_segments(grid(c["z"], de), c["cells"], lab, c["angle"], h * de, w * de, return_cells=True,
                                  return_curve=True, **kw)
    one, ocv = sl.fit_profiles(grid(c["z"], de), c["cells"], c["angle"], h * de, w * de, return_curve=True, **kw)
    order = np.argsort(lab)
    one, ocv = one[order], ocv[order]                                       # in label order
    assert (one["status"] & 1 == 0).sum() >= max(1, K // 4)
    for f in ONE_FIELDS:
        assert seg[f].tobytes() == one[f].tobytes(), (name, f)
    assert cv.tobytes() == ocv.tobytes()
    assert (seg["n_dormant"] == 0).all() and (seg["n_cells"] == 1).all()
    back = one[np.argsort(order)]
    for f in ("cell", "n", "b", "c0", "sse", "loss", "n_down"):
        assert ct[f].tobytes() == back[f].tobytes(), (name, f)


@pytest.mark.parametrize("loss", LOSSES)
def test_two_runs_and_another_order_of_the_segments_return_the_same_rows(loss):
    """5. The same bytes twice, and whole segments in another order the same rows."""
    c = cases(loss)["weights: NaN cells"]
    table, ct, curve = run_case(c)
    again, act, acurve = run_case(c)
    assert again.tobytes() == table.tobytes() and act.tobytes() == ct.tobytes() and acurve.tobytes() == curve.tobytes()
    # the cells grouped by label, the labels in another order, the order inside a label kept
    labs = np.unique(c["labels"])
    perm = np.concatenate([np.flatnonzero(c["labels"] == l) for l in labs[::-1]])
    kw = dict(ages=c["ages"], delta=c["delta"], min_samples=c["min_samples"], min_profiles=c["min_profiles"],
              weights=c["weights"], **c["robust"])
    ptable, pct, pcurve = run(c["z"], c["de"], c["cells"][perm], c["labels"][perm], c["angle"][perm], c["h"], c["w"], **kw)
    assert ptable.tobytes() == table.tobytes() and pcurve.tobytes() == curve.tobytes() and pct.tobytes() == ct[perm].tobytes()
    only = sl.fit_segments(grid(c["z"], c["de"]), c["cells"], c["labels"], c["angle"], c["h"] * c["de"], c["w"] * c["de"], **kw)
    assert only.tobytes() == table.tobytes()                               # the run without the cell table and the curve


# ---- against the restatement ---------------------------------------------------------------------------------------------------
ALL = [(loss, name) for loss in LOSSES for name in NAMES] + [("tukey", "no age survives")]


@pytest.mark.parametrize("loss,name", ALL)
def test_against_the_restatement(loss, name):
    c = cases(loss)[name]
    table, ct, curve = run_case(c)
    ref = reference(loss, name)
    S, A = len(ref), len(c["ages"])
    kept = np.flatnonzero(c["labels"] > 0)
    assert table.dtype == segments.ROBUST_FIT_DTYPE and ct.dtype == segments.ROBUST_CELL_DTYPE
    assert len(table) == S and curve.shape == (S, A) and len(ct) == len(kept)
    nx = c["z"].shape[1]
    assert np.array_equal(ct["cell"], c["cells"][kept]) and np.array_equal(ct["row"] * nx + ct["col"], ct["cell"])
    assert np.array_equal(table["height"], 2.0 * table["a"], equal_nan=True)
    st = qr.compare(c, ref, table, by_position(ct, c), curve)
    print("%s, %s: %s" % (loss, name, st))
    fit = (table["status"] & 1) == 0
    assert np.array_equal(table["rmse"][fit], np.sqrt(table["loss"][fit] / table["dof"][fit]))
    assert np.array_equal(table["kt"][fit], c["ages"][table["kt_index"][fit]])
    assert np.array_equal(curve[fit, table["kt_index"][fit]], table["loss"][fit])
    assert np.isnan(curve[~fit]).all()
    if name == "sizes 1 2 63 64 65 129":
        assert sorted(table["n_profiles"]) == [1, 2, 63, 64, 65, 129] and (table["n_cells"] == table["n_profiles"] + 1).all()
    if name in ("no cell", "labels <= 0 only"):
        assert S == 0 and len(ct) == 0
    if name == "not fitted":
        assert table["status"].tolist()[1:] == [1, 1] and table["n_profiles"].tolist() == [9, 3, 0] and fit[0]
    if name == "no age survives":
        assert (table["status"] == 33).all() and (table["scale"] == 1e-9).all()
    if name in ("borders", "NaN cells", "weights: a strip of zeros"):
        assert int((ct["used"] == 1).sum()) >= 20 and int(((ct["used"] == 1) & (ct["n"] < 2 * c["h"] + 1)).sum()) >= 20
    if name == "block":
        dorm = int(table["n_dormant"][0])
        print("block, %s: %d dormant profiles, index %d" % (loss, dorm, table["kt_index"][0]))
        assert table["kt_index"][0] == qr.BLOCK_GPU_INDEX and c["ages"][qr.BLOCK_GPU_INDEX] == 10.0
        assert dorm == int(ct["dormant"].sum()) and (dorm >= 1 if loss == "tukey" else dorm == 0)


@pytest.mark.parametrize("loss", LOSSES)
def test_zero_scale_returns_the_least_squares_row(loss):
    """A noise-free plane with a dyadic slope, the profiles along the rows (tests/test_gpu_robust.py says why): every
    sample, mean and sum is exact, the residuals are 0 and so is the pooled sigma."""
    n = 96
    z = 0.015625 * np.arange(n, dtype=np.float64)[None, :] * np.ones((n, 1))
    cells = np.array([48 * n + 48, 40 * n + 50, 30 * n + 10, 20 * n + 44, 60 * n + 40])
    lab = np.array([2, 2, 1, 2, 1])
    kw = dict(ages=[1.0, 10.0, 100.0], min_samples=4)
    plain, pct, pcurve = run(z, 1.0, cells, lab, 0.0, 20, 1, **kw)
    got, ct, curve = run(z, 1.0, cells, lab, 0.0, 20, 1, robust=loss, **kw)
    assert (got["scale"] == 0.0).all() and (got["status"] & 16 == 16).all() and (got["n_down"] == 0).all()
    assert (got["n_dormant"] == 0).all()
    for f in SHARED:
        if f != "status":
            assert got[f].tobytes() == plain[f].tobytes(), f
    for f in SHARED_CELL:
        assert ct[f].tobytes() == pct[f].tobytes(), f
    assert np.array_equal(got["status"], plain["status"] | 16) and curve.tobytes() == pcurve.tobytes()
    assert got["loss"].tobytes() == got["sse"].tobytes() and np.array_equal(got["ls_index"], got["kt_index"])
    assert ct["loss"].tobytes() == ct["sse"].tobytes() and (ct["n_down"] == 0).all() and (ct["dormant"] == 0).all()
    # (the longdouble twin: on these inputs Frisch-Waugh is exact as the device's is, LAPACK's lstsq is not)
    ref = qr.fit_segments(z, None, 1.0, cells, lab, 0.0, 20, 1, np.array(kw["ages"]), fit=qr.joint_fw, robust=loss)
    assert [r["status"] for r in ref] == got["status"].tolist() and all(r["scale"] == 0.0 for r in ref)
    assert [r["kt_index"] for r in ref] == got["kt_index"].tolist() and all(r["sse"] == 0.0 for r in ref)


# ---- what the feature is for ----------------------------------------------------------------------------------------------------
def test_the_trench_on_the_device():
    """One segment of 100 profiles with a trench along the strike: least squares dates it two grid steps off and its
    interval does not say so; both losses and the masked plane return the true index."""
    c = qr.trench_case()
    args = (c["z"], c["de"], c["cells"], c["labels"], c["angle"], c["h"], c["w"])
    kw = dict(ages=c["ages"], min_samples=c["min_samples"])
    rows = {"least squares": run(*args, **kw)[0][0]}
    for loss in LOSSES:
        rows[loss] = run(*args, robust=loss, **kw)[0][0]
    rows["masked"] = run(*args, weights=qr.trench_case(mask=True)["weights"], **kw)[0][0]
    for k, r in rows.items():
        print("%-13s index %d, interval [%d, %d], a %.4f%s" % (k, r["kt_index"], r["lo_index"], r["hi_index"], r["a"],
              ", scale %.4f, n_down %d, n_dormant %d" % (r["scale"], r["n_down"], r["n_dormant"]) if k in LOSSES else ""))
        assert r["n_profiles"] == 100 and (r["n"] == 20100 if k != "masked" else 15000 < r["n"] < 20100)
    ls = rows["least squares"]
    assert ls["kt_index"] != qr.TRUE_INDEX and not ls["lo_index"] <= qr.TRUE_INDEX <= ls["hi_index"]
    for k in LOSSES + ("masked",):
        assert (rows[k]["kt_index"], rows[k]["lo_index"], rows[k]["hi_index"]) == (qr.TRUE_INDEX,) * 3, k
        assert rows[k]["ls_index"] == (ls["kt_index"] if k in LOSSES else qr.TRUE_INDEX)


def test_matcher_route_returns_the_module_routes_bytes():
    c = cases("tukey")["weights: random positive"]
    g = grid(c["z"], c["de"])
    labels = np.zeros(c["z"].shape, dtype=np.int32)
    labels.ravel()[c["cells"]] = c["labels"] // 2
    seg = np.zeros(int(labels.max()), dtype=traces.SEGMENT_DTYPE)
    seg["label"], seg["strike"] = np.arange(1, len(seg) + 1), 0.2
    tr = traces.Traces(labels > 0, labels, seg)
    cells = np.flatnonzero(labels.ravel() > 0)
    kw = dict(ages=c["ages"], min_samples=c["min_samples"], weights=c["weights"], robust="tukey", iterations=4,
              return_cells=True, return_curve=True)
    a = sl.Matcher(g).fit_segments(tr, c["h"] * c["de"], c["w"] * c["de"], strike="segment", **kw)
    b = sl.fit_segments(g, cells, labels, 0.2, c["h"] * c["de"], c["w"] * c["de"], **kw)
    assert a[0].dtype == segments.ROBUST_FIT_DTYPE and len(a[0]) == len(np.unique(labels[labels > 0])) >= 3 and (a[0]["status"] & 1 == 0).all()
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_library_refuses_what_the_header_says(gpu_ctx):
    ctx = _lib.Context(0)
    z = pr.synthetic_z(64)
    ages = np.array([1.0, 2.0])
    i64, i32 = (lambda v: np.array(v, dtype=np.int64)), (lambda v: np.array(v, dtype=np.int32))
    base = dict(cells=i64([5 * 64 + 30, 6 * 64 + 30]), sa=np.array([0.0, 0.0]), ca=np.array([1.0, 1.0]), start=i64([0, 1, 2]),
                label=i32([1, 2]), kt=ages, h=10, w=1, de=1.0, delta=1.0, ms=4, mp=1, zz=z, weights=None,
                loss=_lib.ROBUST_HUBER, tuning=1.345, iterations=8, scale=0.0)

    def fit(**kw):
        a = dict(base, **kw)
        return ctx.fit_segments_robust(a["cells"], a["sa"], a["ca"], a["start"], a["label"], a["kt"], a["h"], a["w"], a["de"],
                                       a["delta"], a["ms"], a["mp"], weights=a["weights"], loss=a["loss"], tuning=a["tuning"],
                                       iterations=a["iterations"], scale=a["scale"], cell_table=True, curve=True, z=a["zz"])
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-3\)"):
        fit(zz=None)                                                       # no DEM set
    rows, ct, cv = fit()
    assert list(rows["label"]) == [1, 2] and (rows["status"] & 1 == 0).all() and (ct["used"] == 1).all()
    fit(iterations=64)
    fit(loss=_lib.ROBUST_NONE, tuning=0.0, iterations=0)                   # without a loss its arguments are not read
    for kw in (dict(loss=3), dict(loss=-1), dict(tuning=0.0), dict(tuning=np.nan), dict(tuning=np.inf), dict(iterations=0),
               dict(scale=-1.0), dict(scale=np.nan), dict(ms=1), dict(kt=np.array([2.0, 1.0])), dict(cells=i64([64 * 64, 5])),
               dict(start=i64([0, 2, 1])), dict(start=i64([0, 1, 3])), dict(label=i32([2, 2])), dict(mp=0)):
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-1\)"):
            fit(**kw)
    for kw in (dict(iterations=65), dict(kt=np.arange(1.0, 66.0)), dict(h=1025), dict(w=33)):
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\)"):
            fit(**kw)
    # the largest supported call: Python's cap and the library's refuse the same segment, with and without a plane
    h, A = 1024, 64
    kt = 10 ** np.linspace(0, 3, A)
    for plane in (None, np.ones(z.shape)):
        cap = _lib.segment_robust_cap(h, A, plane is not None)
        assert cap == _lib.SEGMENT_MAX_PARK // (8 * ((2 * h + 1) * (2 if plane is not None else 1) + _lib.SEGMENT_ROBUST_PLANES * A))
        many = dict(cells=np.full(cap + 1, 2080, dtype=np.int64), sa=np.zeros(cap + 1), ca=np.ones(cap + 1), kt=kt, h=h)
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\)"):
            fit(start=i64([0, cap + 1]), label=i32([1]), weights=plane, **many)
        with pytest.raises(ValueError, match="a segment of"):
            sl.fit_segments(grid(z, 1.0), many["cells"], np.ones(cap + 1, dtype=int), 0.0, float(h), ages=kt, weights=plane,
                            robust="huber")
    # empty segments are rows without a fit
    rows, ct, cv = fit(start=i64([0, 0, 2]))
    assert list(rows["n_cells"]) == [0, 2] and list(rows["status"] & 1) == [1, 0] and np.isnan(cv[0]).all()
    rows, ct, cv = fit(cells=i64([]), sa=np.zeros(0), ca=np.zeros(0), start=i64([0, 0, 0]))
    assert list(rows["n_cells"]) == [0, 0] and list(rows["status"]) == [1, 1] and np.isnan(cv).all() and len(ct) == 0
    ctx.close()
