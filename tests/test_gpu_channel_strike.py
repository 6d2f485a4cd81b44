"""sl.fit_channels_along_strike on the MI355X (sc_channel_strike; docs/channels.md, "Width along a reach") against the numpy
restatement (tests/channel_strike_reference.py), in both depth modes: one lstsq per window and frequency on the full design
matrix.

Tolerances are those of tests/test_gpu_channel_segments.py and stand on the same ground: every compared window has a
column-scaled design matrix of condition number <= 1e3 and, with depth="segment" - where the device forms sse_i as SSpp - Q_i
(docs/strike.md, "The subtraction") - SSpp / sse_min <= 1e3, both asserted on the restatement.  Integers, statuses and
dead-frequency masks are equal except in a window one of whose decisions the restatement itself made within 1e-9; such windows
may be at most 1 % of a case, and tests/test_channel_strike_host.py shows that the inputs hold none.  Floats and curves agree
within 1e-9 relative, a within 1e-9 of the window's largest peak-to-peak range.  The anchors and the independence of the
reaches are byte comparisons."""
import contextlib

import numpy as np
import pytest

import channel_reference as cr
import channel_strike_reference as cw
import scarplet_amd as sl
from scarplet_amd import _lib, core, synthetic

pytestmark = pytest.mark.gpu

NAMES = ["run 1", "run 63", "run 64", "run 65", "run 128", "run 129", "run 130", "unusable", "unusable min_profiles 3", "F = 1",
         "F = 64, h = 100, D = 8", "D = 0", "D = h - min_samples", "de = 2", "several reaches", "NaN holes",
         "a hole at the centre at pi f de = 6", "every frequency dead"]


def grid(z, de):
    return sl.DEMGrid.from_array(z, float(de))


def run(case, mode, pick=None, **kw):
    h, w, de = case["h"], case["w"], case["de"]
    pick = slice(None) if pick is None else pick
    args = dict(swath=w * de, window=case["window"], step=case["step"], max_shift=case["D"] * de, depth=mode, delta=case["delta"],
                min_samples=case["min_samples"], min_profiles=case["min_profiles"])
    args.update(kw)
    return sl.fit_channels_along_strike(grid(case["z"], de), case["cells"][pick], case["labels"][pick], case["angle"][pick], h * de,
                                        case["frequencies"], **args)


def case_of(name):
    return cw.gpu_cases()[NAMES.index(name)]


@contextlib.contextmanager
def option(name, value, default):
    ctx = core._context(0)
    ctx.set_option(name, value)
    try:
        yield ctx
    finally:
        ctx.set_option(name, default)


def same_bytes(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def test_the_case_list_is_the_one_named_here():
    assert [c["name"] for c in cw.gpu_cases()] == NAMES == cw.NAMES
    for c in cw.gpu_cases():
        assert max(c["z"].shape) <= 300 and len(c["cells"]) <= 300


# ---- 1. against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", cw.MODES)
@pytest.mark.parametrize("name", NAMES)
def test_against_the_restatement(name, mode):
    case = case_of(name)
    table, curve = run(case, mode, return_curve=True)
    F = len(case["frequencies"])
    assert curve.shape == (len(table), F) and curve.dtype == np.float64
    ref = cw.restate(case, mode)
    st = cw.compare(ref, mode, table, curve, case["de"])
    print("%s, %s: %s" % (name, mode, st))
    assert st["ties"] == 0                                                 # (the restatement alone needs none: the host test)
    fit = table["status"] & 1 == 0
    prof, ncell, status = table["n_profiles"], table["n_cells"], table["status"]
    assert np.array_equal(table["f"][fit], case["frequencies"][table["f_index"][fit]])
    want = cr.derived(table["f"][fit], table["f_lo"][fit], table["f_hi"][fit], table["a"][fit])
    for f, v in want.items():
        assert np.allclose(table[f][fit], v, rtol=1e-14, atol=0), f
    assert np.isnan(table["shift_mean"][~fit]).all() and (np.abs(table["shift_mean"][fit]) <= case["D"] * case["de"]).all()
    if mode == "profile":
        assert np.array_equal(table["dof"], table["n"] - (3 + (case["D"] > 0)) * prof)
    else:
        assert np.array_equal(table["dof"], table["n"] - 2 * prof - 1 - (prof if case["D"] > 0 else 0))
    # the table is sorted by (label, station)
    key = table["label"].astype(np.int64) * (1 << 32) + table["station"]
    assert (np.diff(key) > 0).all()
    if name.startswith("run"):
        assert int(name.split()[1]) in prof.tolist() and fit.all(), prof
    if name.startswith("unusable"):
        assert ((ncell == 0) & (status == 1)).any()                        # an empty window
        assert ((ncell > 0) & (prof == 0)).any()                           # cells, none usable
        assert ((prof > 0) & (prof < ncell) & fit).any()                   # some unusable in a run
        assert ((prof >= 1) & (table["dof"] < 1) & (status == 1)).any()    # dof < 1
        assert np.isnan(table["row"][ncell == 0]).all() and not np.isnan(table["row"][ncell > 0]).any()
        sparse = (prof > 0) & (prof < 3) & (table["dof"] >= 1)
        assert sparse.any() and ((status[sparse] == 1) == (case["min_profiles"] == 3)).all()
        assert sorted(set(table["label"].tolist())) == [3, 7, 9]
    if name == "F = 1":
        assert F == 1 and (status[fit] & 6 == 6).all() and (table["f_index"][fit] == 0).all()
    if name == "F = 64, h = 100, D = 8":
        assert F == 64
    if name == "D = 0":
        assert not (status & 8).any() and not table["shift_mean"][fit].any()
    if name == "several reaches":
        assert sorted(set(table["label"].tolist())) == [2, 5, 9, 11] and np.any(np.diff(case["labels"]) < 0)
        one = table[table["label"] == 11]
        assert len(one) == 1 and one["n_cells"][0] == 1 and one["station"][0] == 0
    if name == "a hole at the centre at pi f de = 6":
        holed = np.array([40 in (case["cells"][r["where"]] // 128) for r in ref])
        assert holed.any() and not holed.all() and fit.all()
        assert np.array_equal(np.isnan(curve[:, F - 1]), holed) and not np.isnan(curve[:, :F - 1]).any()
    if name == "every frequency dead":
        holed = np.array([40 in (case["cells"][r["where"]] // 128) for r in ref])
        assert np.array_equal(status, np.where(holed, 33, 6)) and holed.any() and not holed.all()
    # a second run and the run without the curve: the same bytes
    same_bytes(run(case, mode, return_curve=True), (table, curve))
    assert run(case, mode).tobytes() == table.tobytes()


# ---- 2. anchors, bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", cw.MODES)
def test_one_window_over_a_reach_is_fit_channel_segments(mode):
    """A window that holds the whole reach, whose input order is its order along the strike: the sums have the shape of
    fit_channel_segments' - runs of 64 from the first usable profile.  200 cells: four runs.  With depth="profile" the row and
    the curve are its bytes; with depth="segment" f_index and a are (its sse is that of explicit residuals)."""
    case = case_of("run 130")
    assert (np.diff(case["cells"] // 300) > 0).all()
    row, curve = run(case, mode, window=400.0, step=400.0, return_curve=True)
    h, w, de = case["h"], case["w"], case["de"]
    fit, cv = sl.fit_channel_segments(grid(case["z"], de), case["cells"], case["labels"], case["angle"], h * de, case["frequencies"],
                                      swath=w * de, max_shift=case["D"] * de, depth=mode, delta=case["delta"],
                                      min_samples=case["min_samples"], return_curve=True)
    assert len(row) == 1 and len(fit) == 1 and row["n_profiles"][0] == 200 and fit["status"][0] & 1 == 0
    for f in ("label", "n_cells", "n_profiles", "n", "dof", "f_index", "f", "a", "depth"):
        assert row[f].tobytes() == fit[f].tobytes(), f
    if mode == "profile":
        for f in ("lo_index", "hi_index", "status", "f_lo", "f_hi", "sse", "rmse", "width", "width_lo", "width_hi", "area"):
            assert row[f].tobytes() == fit[f].tobytes(), f
        assert curve.tobytes() == cv.tobytes()
    else:
        assert abs(row["sse"][0] - fit["sse"][0]) <= 1e-9 * fit["sse"][0]
        assert (row["status"][0] & 8) == (fit["status"][0] & 8)


@pytest.mark.parametrize("mode", cw.MODES)
def test_a_window_of_one_profile_is_fit_channels(mode):
    """Windows of one cell each (window = step = the cell size on a column): f_index and a are fit_channels' for that cell,
    bit for bit - one profile is no addition at all -, and shift_mean is its shift; with depth="profile" so are lo_index,
    hi_index, status, sse and rmse."""
    case = case_of("run 1")
    table = run(case, mode)
    h, w, de = case["h"], case["w"], case["de"]
    one = sl.fit_channels(grid(case["z"], de), case["cells"], case["angle"], h * de, case["frequencies"], swath=w * de,
                          max_shift=case["D"] * de, delta=case["delta"], min_samples=case["min_samples"])
    assert len(table) == 200 and (table["n_profiles"] == 1).all() and (one["status"] & 1 == 0).all()
    assert np.array_equal(table["row"] * 300 + table["col"], case["cells"])
    for f in ("f_index", "f", "a", "depth", "n"):
        assert table[f].tobytes() == one[f].tobytes(), f
    assert np.array_equal(table["shift_mean"], one["shift"])
    if mode == "profile":
        for f in ("lo_index", "hi_index", "status", "sse", "rmse", "width_lo", "width_hi"):
            assert table[f].tobytes() == one[f].tobytes(), f
        assert np.array_equal(table["dof"], one["n"] - 4)
    else:
        assert (np.abs(table["sse"] - one["sse"]) <= 1e-9 * one["sse"]).all()
        assert np.array_equal(table["status"] & 8, one["status"] & 8)


# ---- 3. determinism and routes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", cw.MODES)
def test_the_terms_planes_change_no_byte(mode):
    """Both routes of stage one in one window ("NaN holes": complete and incomplete profiles): the rows with option
    "channel_terms" 1 and 0 are the same bytes."""
    case = case_of("NaN holes")
    with option("channel_terms", 0, 1):
        a = run(case, mode, return_curve=True)
    same_bytes(a, run(case, mode, return_curve=True))


@pytest.mark.parametrize("mode", cw.MODES)
@pytest.mark.parametrize("name", ["several reaches", "unusable", "run 130"])
def test_the_same_bytes_for_every_chunking(name, mode):
    case = case_of(name)
    a = run(case, mode, return_curve=True)
    for n in (1, 70):
        with option("fit_chunk", n, 0):
            same_bytes(run(case, mode, return_curve=True), a)


@pytest.mark.parametrize("mode", cw.MODES)
def test_a_reach_does_not_depend_on_the_others(mode):
    """Each reach's rows are the same bytes whether it is passed alone or with the others, in shuffled order."""
    case = case_of("several reaches")
    table, curve = run(case, mode, return_curve=True)
    for L in np.unique(table["label"]):
        t1, c1 = run(case, mode, pick=case["labels"] == L, return_curve=True)
        rows = table["label"] == L
        assert t1.tobytes() == table[rows].tobytes() and c1.tobytes() == curve[rows].tobytes(), L


def test_the_matcher_route_gives_the_same_bytes():
    g = synthetic.synthetic_channel(256)
    m = sl.Matcher(g)
    f0 = 0.035
    m.search(sl.Channel, 50.0, [f0], np.linspace(-0.3, 0.3, 9))
    res = np.array(m.result_array())
    top = float(np.nanmax(res[3]))
    tr = m.extract_traces(0.25 * top, 0.5 * top, 4)
    cells = np.flatnonzero(tr.labels.ravel() > 0)
    assert 20 < len(cells) <= 600 and len(tr.segments) >= 1
    fs = f0 * 1.12 ** np.arange(-6, 7)
    for mode in cw.MODES:
        kw = dict(swath=2.0, max_shift=3.0, depth=mode, return_curve=True)
        a = m.fit_channels_along_strike(tr, 30.0, fs, 40.0, step=10.0, **kw)
        b = sl.fit_channels_along_strike(g, cells, tr.labels, res[2], 30.0, fs, window=40.0, step=10.0, **kw)
        same_bytes(a, b)
        assert np.array_equal(np.unique(a[0]["label"]), tr.segments["label"]) and (a[0]["status"] & 1 == 0).any()
        d = m.fit_channels_along_strike(tr, 30.0, fs, 40.0, step=10.0, strike="segment", **kw)
        e = sl.fit_channels_along_strike(g, cells, tr.labels, tr.segments["strike"][tr.labels.ravel()[cells] - 1], 30.0, fs,
                                         window=40.0, step=10.0, **kw)
        same_bytes(d, e)
    # the search's record is what it was
    assert np.array_equal(np.array(m.result_array()), res, equal_nan=True)


# ---- 4. the recovery ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", cw.MODES)
def test_the_recovery_is_the_restatements(mode):
    """docs/channels.md, "Width along a reach": on the trough that doubles its width along the reach the eleven stations
    return the planted widths of their own cells, every interval one frequency wide."""
    case = cw.recovery(3)
    table, curve = run(case, mode, return_curve=True)
    st = cw.compare(cw.restate(case, mode), mode, table, curve, case["de"])
    print("recovery, %s: %s" % (mode, st))
    assert st["ties"] == 0 and table["n_profiles"].tolist() == cw.REC_PROFILES
    assert table["f_index"].tolist() == cw.REC_INDEX[3] == [16, 15, 15, 14, 14, 13, 12, 12, 11, 11, 10]
    assert np.array_equal(table["lo_index"], table["f_index"]) and np.array_equal(table["hi_index"], table["f_index"])
    assert (np.diff(table["width"]) >= 0).all() and table["width"][-1] > 1.9 * table["width"][0]


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def test_library_refuses_what_the_header_says(gpu_ctx):
    ctx = _lib.Context(0)
    z = cr.channel_z(64)
    fs = np.array([0.05, 0.1])
    i64, i32 = (lambda v: np.array(v, dtype=np.int64)), (lambda v: np.array(v, dtype=np.int32))
    cells, sa, ca = i64([5 * 64 + 30, 6 * 64 + 30, 7 * 64 + 30]), np.zeros(3), np.ones(3)
    base = dict(sws=(0, 1, 2), lo=(0, 2), hi=(2, 3), D=2, seg=(0, 2, 3), f=fs, mode=0, zz=z, label=(1, 2), mp=1, h=10)

    def fit(**kw):
        a = dict(base, **kw)
        return ctx.channel_strike(cells, sa, ca, i64(a["seg"]), i32(a["label"]), i64(a["sws"]), i64(a["lo"]), i64(a["hi"]), a["f"],
                                  a["h"], 1, a["D"], a["mode"], 1.0, 1.0, 4, a["mp"], curve=True, z=a["zz"])
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-3\)"):
        fit(zz=None)                                                       # no DEM set
    rows, cv, ss = fit()
    assert rows["n_cells"].tolist() == [2, 1] and (rows["status"] & 1 == 0).all() and rows["station"].tolist() == [0, 0]
    assert rows["label"].tolist() == [1, 2] and cv.shape == (2, 2) and (np.abs(ss) <= 2 * rows["n_profiles"]).all()
    empty = fit(lo=(1, 3), hi=(1, 3))                                      # empty windows are allowed
    assert empty[0]["n_cells"].tolist() == [0, 0] and (empty[0]["status"] == 1).all() and np.isnan(empty[1]).all()
    # what sc_fit_strike refuses of the window arrays, and what sc_channel_segments refuses
    for kw in (dict(lo=(0, 1)), dict(hi=(3, 3)), dict(lo=(2, 2), hi=(1, 3)), dict(sws=(0, 1, 1)), dict(sws=(1, 1, 2)),
               dict(sws=(0, 2, 1)), dict(D=-1), dict(D=7), dict(seg=(0, 2, 2)), dict(mode=2), dict(mode=-1), dict(mp=0),
               dict(f=np.array([0.1, 0.05])), dict(f=np.array([0.0, 0.1])), dict(f=np.array([0.05, 6.001 / np.pi])),
               dict(f=np.array([])), dict(label=(2, 2)), dict(label=(0, 1))):
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-1\)"):
            fit(**kw)
    for kw in (dict(f=np.linspace(0.01, 0.02, 65)), dict(h=1025)):
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\)"):
            fit(**kw)
    # null pointers: straight at the library
    lib = ctx.lib
    assert len(_lib.SIGNATURES["sc_channel_strike_dem"][1]) == 28
    assert lib.sc_channel_strike_dem(None, None, 0, 0, None, None, None, 0, None, None, 0, None, None, None, 0, None, 0, 1, 0, 0, 0,
                                     1.0, 1.0, 1, 1, None, None, None) == -1
    assert lib.sc_channel_strike(None, None, None, None, 0, None, None, 0, None, None, None, 0, None, 0, 1, 0, 0, 0, 1.0, 1.0, 1, 1,
                                 None, None, None) == -1
    assert fit()[0].tobytes() == rows.tobytes()
    ctx.close()
