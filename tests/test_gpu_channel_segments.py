"""sl.fit_channel_segments on the MI355X (sc_channel_segments; docs/channels.md, "One width per reach") against the numpy
restatement (tests/channel_segment_reference.py), in both depth modes.

Tolerances are those of tests/test_gpu_channels.py and tests/test_gpu_segments.py and stand on the same ground: every
compared joint fit has a column-scaled design matrix of condition number <= 1e3 (asserted on the restatement), and the
restatement agrees with a longdouble one within 1e-11 on every input here (tests/test_channel_segments_host.py), so the pooled
curves and every profile's share agree within 1e-9 relative and c0, b h de, a within 1e-9 of the reach's largest peak-to-peak
range.  Integers, statuses and shifts are equal except in a reach one of whose decisions the restatement itself made within
1e-9; such reaches may be at most 1 % of a case, and the host test shows that the inputs hold none within 1e-8.  The anchors
are byte comparisons.
"""
import contextlib

import numpy as np
import pytest

import channel_reference as cr
import channel_segment_reference as csr
import scarplet_amd as sl
from scarplet_amd import _lib, core, synthetic, traces

pytestmark = pytest.mark.gpu

NAMES = ["sizes 1 2 63 64 65 129, h = 8, labels <= 0", "unusable cells, none usable, min_profiles 3, dof < 1", "F = 1",
         "F = 35, D = 8", "F = 64, h = 100, D = 8", "D = 0", "D = h - min_samples", "de = 2", "NaN cells",
         "a hole at the centre at pi f de = 6", "every frequency dead"]
ALL = dict(return_cells=True, return_curve=True, return_shift=True)


def grid(z, de):
    return sl.DEMGrid.from_array(z, float(de))


def run(case, mode, **kw):
    h, w, de = case["h"], case["w"], case["de"]
    return sl.fit_channel_segments(grid(case["z"], de), case["cells"], case["labels"], case["angle"], h * de, case["frequencies"],
                                   swath=w * de, max_shift=case["D"] * de, depth=mode, delta=case["delta"],
                                   min_samples=case["min_samples"], min_profiles=case["min_profiles"], **kw)


def single(case, pos, **kw):
    """sl.fit_channels on the cells of the case at the input positions ``pos``, with the case's options."""
    h, w, de = case["h"], case["w"], case["de"]
    return sl.fit_channels(grid(case["z"], de), case["cells"][pos], case["angle"][pos], h * de, case["frequencies"], swath=w * de,
                           max_shift=case["D"] * de, delta=case["delta"], min_samples=case["min_samples"], **kw)


def case_of(name):
    return csr.gpu_cases()[NAMES.index(name)]


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
    assert [c["name"] for c in csr.gpu_cases()] == NAMES
    for c in csr.gpu_cases():
        assert max(c["z"].shape) <= 600 and len(c["cells"]) <= 400
        assert 0 <= c["D"] <= min(_lib.PROFILE_MAX_SHIFT, c["h"] - c["min_samples"])


# ---- 1. against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", csr.MODES)
@pytest.mark.parametrize("name", NAMES)
def test_against_the_restatement(name, mode):
    case = case_of(name)
    table, ct, curve, shifts = run(case, mode, **ALL)
    kept = np.flatnonzero(case["labels"] > 0)
    S, F = len(np.unique(case["labels"][kept])), len(case["frequencies"])
    assert len(table) == S and curve.shape == (S, F) and shifts.shape == (len(kept), F) and shifts.dtype == np.int8
    nx = case["z"].shape[1]
    assert np.array_equal(ct["cell"], case["cells"][kept]) and np.array_equal(ct["row"] * nx + ct["col"], ct["cell"])
    assert np.array_equal(ct["label"], case["labels"][kept])
    ref = csr.restate(case, mode)
    st = csr.compare(ref, mode, table, ct, curve, shifts, kept, case["h"], case["de"], case["D"])
    print("%s, %s: %s" % (name, mode, st))
    fit = table["status"] & 1 == 0
    freqs = case["frequencies"]
    assert np.array_equal(table["f"][fit], freqs[table["f_index"][fit]])
    assert np.array_equal(curve[fit, table["f_index"][fit]], table["sse"][fit])
    assert np.abs(shifts).max(initial=0) <= case["D"]
    want = cr.derived(table["f"][fit], table["f_lo"][fit], table["f_hi"][fit], table["a"][fit])
    for f, v in want.items():
        assert np.allclose(table[f][fit], v, rtol=1e-14, atol=0), f
    ok = ~np.isnan(ct["b"])
    sa, ca = np.sin(case["angle"][kept]), np.cos(case["angle"][kept])
    assert np.array_equal(ct["centre_row"][ok], (ct["row"] - ct["shift_index"] * sa)[ok])
    assert np.array_equal(ct["centre_col"][ok], (ct["col"] + ct["shift_index"] * ca)[ok])
    assert np.array_equal(ct["shift"][ok], ct["shift_index"][ok] * case["de"])
    by = {int(r["label"]): r for r in table}
    if name == NAMES[0]:
        assert sorted(table["n_profiles"]) == [1, 2, 63, 64, 65, 129] and fit.all()
    elif name == NAMES[1]:
        assert [int(by[l]["status"]) & 1 for l in (1, 3, 4, 6, 8)] == [1, 0, 0, 1, 1]
        assert int(by[6]["n"]) == 4 and int(by[6]["dof"]) < 1 and int(by[8]["n_profiles"]) == 2 and int(by[1]["n_profiles"]) == 0
    elif name == "D = 0":
        assert not (table["status"] & 8).any() and not shifts.any()
    elif name == "a hole at the centre at pi f de = 6":
        assert list(np.flatnonzero(np.isnan(curve[0]))) == [F - 1] and not np.isnan(curve[1]).any() and fit.all()
    elif name == "every frequency dead":
        assert list(table["status"]) == [33, 6] and np.isnan(curve[0]).all()
    if mode == "segment":
        # the reach's amplitude in every usable row of its cells
        for r in table[fit]:
            rows = (ct["label"] == r["label"]) & (ct["used"] == 1)
            assert np.all(ct["a"][rows] == r["a"])
    # the runs without the optional outputs: the same bytes
    assert run(case, mode).tobytes() == table.tobytes()
    same_bytes(run(case, mode, return_curve=True), (table, curve))


# ---- 2. anchors, bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", csr.MODES)
@pytest.mark.parametrize("name", ["sizes 1 2 63 64 65 129, h = 8, labels <= 0", "F = 35, D = 8", "NaN cells", "D = 0",
                                  "every frequency dead"])
def test_a_reach_of_one_usable_profile_is_fit_channels(name, mode):
    """Every cell of the case as a reach of its own: a usable one returns f_index, lo_index, hi_index, status, a, sse, rmse of
    sl.fit_channels for that cell, and its b, c0, shift_index in the cell table; the curve and the shifts are its own too."""
    case = case_of(name)
    K = len(case["cells"])
    one = dict(case, labels=np.arange(1, K + 1, dtype=np.int64))
    table, ct, curve, shifts = run(one, mode, **ALL)
    rows, cv, sp = single(case, np.arange(K), return_curve=True, return_shift=True)
    usable = ct["used"] == 1
    assert usable.sum() >= 3
    for f in ("f_index", "lo_index", "hi_index", "status", "f", "f_lo", "f_hi", "a", "sse", "rmse", "depth", "width", "area"):
        assert table[f][usable].tobytes() == rows[f][usable].tobytes(), f
    for f in ("a", "b", "c0", "sse", "shift_index", "shift", "n", "centre_row", "centre_col"):
        assert ct[f][usable].tobytes() == rows[f][usable].tobytes(), f
    assert curve[usable].tobytes() == cv[usable].tobytes() and shifts[usable].tobytes() == sp[usable].tobytes()
    assert np.all(table["status"][~usable] == 1) and np.all(table["n_profiles"] == usable)
    if name == "every frequency dead":
        assert list(table["status"]) == [6, 33, 6, 6]


@pytest.mark.parametrize("name", ["sizes 1 2 63 64 65 129, h = 8, labels <= 0", "NaN cells", "F = 64, h = 100, D = 8",
                                  "a hole at the centre at pi f de = 6"])
def test_profile_mode_is_the_blocked_sum_of_fit_channels_curves(name):
    case = case_of(name)
    table, ct, curve, shifts = run(case, "profile", **ALL)
    kept = np.flatnonzero(case["labels"] > 0)
    rows, cv, sp = single(case, kept, return_curve=True, return_shift=True)
    usable = ct["used"] == 1
    assert shifts[usable].tobytes() == sp[usable].tobytes() and not shifts[~usable].any()
    for s, r in enumerate(table):
        mine = np.flatnonzero((ct["label"] == r["label"]) & usable)
        if r["status"] & 1 and r["status"] != 33:
            continue
        assert len(mine) == r["n_profiles"]
        assert curve[s].tobytes() == csr.blocked_sum(cv[mine]).tobytes(), r["label"]
        if r["status"] & 1 == 0:
            # ... and the row's a the mean of the cells' own, in the same order of additions
            assert r["a"] == csr.blocked_sum(ct["a"][mine][:, None])[0] / len(mine)
            assert r["sse"] == csr.blocked_sum(ct["sse"][mine][:, None])[0]


@pytest.mark.parametrize("mode", csr.MODES)
@pytest.mark.parametrize("name", ["NaN cells", "F = 35, D = 8"])
def test_the_terms_planes_change_no_byte(name, mode):
    case = case_of(name)
    with option("channel_terms", 0, 1):
        a = run(case, mode, **ALL)
    b = run(case, mode, **ALL)
    same_bytes(a, b)


@pytest.mark.parametrize("mode", csr.MODES)
@pytest.mark.parametrize("name", ["sizes 1 2 63 64 65 129, h = 8, labels <= 0", "NaN cells", "F = 64, h = 100, D = 8"])
def test_the_same_bytes_every_way(name, mode):
    case = case_of(name)
    a = run(case, mode, **ALL)
    same_bytes(run(case, mode, **ALL), a)                                   # two runs
    # whole reaches in another order: the labels renumbered in reverse, the cells of a reach in their order
    top = int(case["labels"].max()) + 1
    other = np.where(case["labels"] > 0, top - case["labels"], case["labels"])
    b = run(dict(case, labels=other), mode, **ALL)
    assert len(b[0]) == len(a[0]) > 1
    for f in a[0].dtype.names:
        if f != "label":
            assert a[0][f].tobytes() == b[0][f][::-1].tobytes(), f
    for f in a[1].dtype.names:
        if f != "label":
            assert a[1][f].tobytes() == b[1][f].tobytes(), f
    assert a[2].tobytes() == b[2][::-1].tobytes() and a[3].tobytes() == b[3].tobytes()
    # several chunks of whole reaches
    for n in (1, 70):
        with option("fit_chunk", n, 0):
            same_bytes(run(case, mode, **ALL), a)


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
    for mode in csr.MODES:
        kw = dict(swath=2.0, max_shift=3.0, depth=mode, **ALL)
        a = m.fit_channel_segments(tr, 30.0, fs, **kw)
        b = sl.fit_channel_segments(g, cells, tr.labels, res[2], 30.0, fs, **kw)
        same_bytes(a, b)
        assert np.array_equal(a[0]["label"], tr.segments["label"]) and np.array_equal(a[0]["n_cells"], tr.segments["n_cells"])
        assert (a[0]["status"] & 1 == 0).any()
        d = m.fit_channel_segments(tr, 30.0, fs, strike="segment", **kw)
        e = sl.fit_channel_segments(g, cells, tr.labels, tr.segments["strike"][tr.labels.ravel()[cells] - 1], 30.0, fs, **kw)
        same_bytes(d, e)
    # the search's record is what it was
    assert np.array_equal(np.array(m.result_array()), res, equal_nan=True)
    assert isinstance(tr, traces.Traces)


# ---- 3. the negated surface --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", csr.MODES)
@pytest.mark.parametrize("name", ["F = 35, D = 8", "NaN cells", "sizes 1 2 63 64 65 129, h = 8, labels <= 0"])
def test_the_negated_surface_negates_the_amplitude(name, mode):
    case = case_of(name)
    a = run(case, mode, **ALL)
    b = run(dict(case, z=-case["z"]), mode, **ALL)
    for f in ("f_index", "lo_index", "hi_index", "status", "n", "dof", "sse", "rmse"):
        assert a[0][f].tobytes() == b[0][f].tobytes(), f
    assert np.array_equal(a[0]["a"], -b[0]["a"], equal_nan=True) and np.array_equal(a[1]["a"], -b[1]["a"], equal_nan=True)
    assert a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()


# ---- 4. the recovery ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", csr.MODES)
def test_the_recovery_is_the_restatements(mode):
    """docs/channels.md: at noise 0.5 the single cells find the true index in 49 of 100 cells; the reach finds it, with the
    restatement's interval; without the shift both land where the restatement lands."""
    for D in (None, 0):
        case = csr.recovery(D=D)
        table = run(case, mode)
        r = csr.restate(case, mode)[0]
        assert len(table) == 1
        got = tuple(int(table[f][0]) for f in ("f_index", "lo_index", "hi_index", "status", "n", "dof", "n_profiles"))
        assert got == (r["f_index"], r["lo_index"], r["hi_index"], r["status"], r["n"], r["dof"], 100), (D, got)
        assert abs(table["sse"][0] - r["sse"]) <= csr.RTOL * r["sse"] and abs(table["a"][0] - r["a"]) <= csr.RTOL * r["ptp"]
        if D is None:
            assert got[0] == cr.REC["index"]
            rows = single(case, np.arange(100))
            assert int((rows["f_index"] == cr.REC["index"]).sum()) == csr.single_cell_hits(case) < 50


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def test_library_refuses_what_the_header_says(gpu_ctx):
    ctx = _lib.Context(0)
    z = cr.channel_z(64)
    fs = np.array([0.05, 0.1])
    i64, i32 = (lambda v: np.array(v, dtype=np.int64)), (lambda v: np.array(v, dtype=np.int32))
    base = dict(cells=i64([5 * 64 + 30, 6 * 64 + 30]), sa=np.array([0.0, 0.0]), ca=np.array([1.0, 1.0]), start=i64([0, 1, 2]),
                label=i32([1, 2]), f=fs, h=10, w=1, D=2, mode=0, de=1.0, delta=1.0, ms=4, mp=1, zz=z)

    def fit(**kw):
        a = dict(base, **kw)
        return ctx.channel_segments(a["cells"], a["sa"], a["ca"], a["start"], a["label"], a["f"], a["h"], a["w"], a["D"], a["mode"],
                                    a["de"], a["delta"], a["ms"], a["mp"], cell_table=True, curve=True, shift_plane=True, z=a["zz"])
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-3\)"):
        fit(zz=None)                                                       # no DEM set
    rows, ct, cv, sp = fit()
    assert list(rows["label"]) == [1, 2] and (rows["status"] & 1 == 0).all() and (ct["used"] == 1).all()
    for kw in (dict(cells=i64([64 * 64, 5])), dict(sa=np.array([np.nan, 0.0])), dict(f=np.array([0.1, 0.05])),
               dict(f=np.array([0.0, 0.1])), dict(f=np.array([0.05, np.inf])), dict(f=np.array([0.05, 6.001 / np.pi])),
               dict(f=np.array([0.05, 3.0001 / np.pi]), de=2.0), dict(f=np.array([])), dict(ms=11), dict(delta=-1.0),
               dict(zz=z[:1].copy()), dict(de=0.0), dict(D=-1), dict(D=7), dict(mode=2), dict(mode=-1),
               dict(start=i64([0, 2, 1])), dict(start=i64([1, 1, 2])), dict(start=i64([0, 1, 3])),
               dict(label=i32([0, 1])), dict(label=i32([2, 2])), dict(label=i32([3, 2])), dict(mp=0)):
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-1\)"):
            fit(**kw)
    for kw in (dict(f=np.linspace(0.01, 0.02, 65)), dict(h=1025), dict(w=33), dict(h=100, D=65)):
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\)"):
            fit(**kw)
    fit(f=np.array([0.05, 6.0 / np.pi]))                                   # pi f de = 6 is taken
    # null pointers: straight at the library
    lib, h = ctx.lib, ctx._h
    args = _lib.SIGNATURES["sc_channel_segments_dem"][1]
    assert len(args) == 25
    assert lib.sc_channel_segments_dem(None, None, 0, 0, None, None, None, 0, None, None, 0, None, 0, 1, 0, 0, 0, 1.0, 1.0, 1, 1,
                                       None, None, None, None) == -1
    assert lib.sc_channel_segments(None, None, None, None, 0, None, None, 0, None, 0, 1, 0, 0, 0, 1.0, 1.0, 1, 1, None, None, None,
                                   None) == -1
    good = fit()
    for drop in ("cells", "sa", "ca", "start", "label", "f", "rows"):
        a = dict(base)
        arr = {k: np.ascontiguousarray(v) for k, v in a.items() if isinstance(v, np.ndarray)}
        ptr = lambda k, t: None if k == drop else arr[k].ctypes.data_as(t)
        out = np.zeros(2, dtype=_lib.SEGMENT_FIT_DTYPE)
        rc = lib.sc_channel_segments_dem(h, arr["zz"].ctypes.data_as(_lib._dp), 64, 64, ptr("cells", _lib._llp), ptr("sa", _lib._dp),
                                         ptr("ca", _lib._dp), 2, ptr("start", _lib._llp), ptr("label", _lib._ip), 2,
                                         ptr("f", _lib._dp), 2, 10, 1, 2, 0, 1.0, 1.0, 4, 1, None if drop == "rows" else out.ctypes.data, None, None, None)
        assert rc == -1, drop
    assert fit()[0].tobytes() == good[0].tobytes()
    # the largest supported call: a reach whose park passes SC_SEGMENT_MAX_PARK bytes
    hh, F = 1024, 64
    big = _lib.channel_segment_cap(hh, F) + 1
    f64 = np.geomspace(0.001, 0.1, F)
    many = dict(cells=np.full(big, 2080, dtype=np.int64), sa=np.zeros(big), ca=np.ones(big), f=f64, h=hh, D=0)
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\).*a segment of"):
        fit(start=i64([0, big]), label=i32([1]), **many)
    with pytest.raises(ValueError, match="a segment of"):
        sl.fit_channel_segments(grid(z, 1.0), many["cells"], np.ones(big, dtype=int), 0.0, float(hh), f64)
    # empty reaches are rows without a fit
    rows, ct, cv, sp = fit(start=i64([0, 0, 2]))
    assert list(rows["n_cells"]) == [0, 2] and list(rows["status"] & 1) == [1, 0] and np.isnan(cv[0]).all()
    # a context that holds a block of a larger grid
    zb = np.ascontiguousarray(z[:40, :])
    ax = np.arange(64.0)
    ctx.set_dem(zb, 1.0, 1.0, ax, ax, origin=(0, 0), shape=(64, 64), core=(0, 32, 0, 64), wrap=False)
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\)"):
        fit(zz=None)
    ctx.close()
