"""sl.bootstrap_along_strike on the MI355X (sc_strike_bootstrap, docs/strike.md "Intervals per station") against the numpy
restatement (tests/strike_bootstrap_reference.py) on the 300 x 300 synthetic surfaces of strike_reference, h = 20.

Integers - n_blocks, n_profiles, n_failed, the histogram, kt_index0, lo_index and hi_index - match the restatement
exactly: the blocks and the draws are integer arithmetic, and a replicate's age is an argmax without a subtraction.  The
one exception is a window that holds a replicate whose two largest Q_i the restatement finds within 1e-12 relative: such
replicates may be at most 0.1 % of a case (strike_bootstrap_reference.compare asserts bootstrap_reference's cap; the
seeds and the noise of the cases were chosen on the CPU so that none has one).  Floats agree within 1e-9 relative, the
family's tolerance.  The anchors, the chunks and the independence of segments are comparisons with the library's other
calls or of bytes."""
import numpy as np
import pytest

import scarplet_amd as sl
import strike_bootstrap_reference as sbr
from scarplet_amd import _lib, _plan, strike_bootstrap, synthetic

pytestmark = pytest.mark.gpu

CASES = REFS = None
NAMES = ["runs", "R 1", "R 1000", "R 4096", "one age", "64 ages", "level 0.5", "level 0.999", "70 blocks", "min_blocks", "a hole",
         "a NaN block", "several segments", "D 3"]


def cases():
    global CASES
    if CASES is None:
        CASES = {c["name"]: c for c in sbr.gpu_cases()}
    return CASES


def ref_of(name):
    """The restatement of a case, computed once and left unchanged."""
    global REFS
    REFS = REFS or {}
    if name not in REFS:
        REFS[name] = sbr.restate(cases()[name])
    return REFS[name]


def grid(z):
    return sl.DEMGrid.from_array(z, 1.0)


def options(case, **kw):
    args = dict(window=case["window"], step=case["step"], block_length=case["block_length"], replicates=case["R"],
                level=case["level"], seed=case["seed"], ages=case["ages"], min_samples=case["min_samples"],
                min_profiles=case["min_profiles"], min_blocks=case["min_blocks"], max_shift=float(case["D"]) if case["D"] else None)
    args.update(kw)
    return args


def run(case, cells=None, labels=None, angle=None, **kw):
    return sl.bootstrap_along_strike(grid(case["z"]), case["cells"] if cells is None else cells,
                                     case["labels"] if labels is None else labels, case["angle"] if angle is None else angle,
                                     float(case["h"]), float(case["w"]), **options(case, **kw))


def test_the_case_list_is_the_one_named_here():
    assert list(cases()) == NAMES
    for c in cases().values():
        assert c["z"].shape == (sbr.N, sbr.N) and len(c["cells"]) <= 600


@pytest.mark.parametrize("name", NAMES)
def test_against_the_restatement(name):
    case = cases()[name]
    table, hist = run(case, return_hist=True)
    ref = ref_of(name)
    A, R = len(case["ages"]), case["R"]
    assert len(table) == len(ref) and hist.shape == (len(ref), A) and hist.dtype == np.int32
    st = sbr.compare(ref, table, hist)
    print("%s: %s" % (name, st))
    done = table["status"] != 1
    assert done.any()
    assert np.array_equal(table["kt0"][done], case["ages"][table["kt_index0"][done]])
    assert np.array_equal(table["kt_lo"][done], case["ages"][table["lo_index"][done]])
    assert np.array_equal(table["kt_hi"][done], case["ages"][table["hi_index"][done]])
    assert (hist.sum(axis=1)[done] == R - table["n_failed"][done]).all() and not hist[~done].any()
    nb = table["n_blocks"]
    if name == "runs":
        # the first block of segment c holds c usable profiles, the second three: sums of one profile, of a run less
        # one, of a run, of a run and one, of two runs and one
        assert table["label"].tolist() == [1, 2, 3, 4, 5] and (table["station"] == 0).all() and (nb == 2).all()
        assert table["n_profiles"].tolist() == [c + 3 for c in sbr.RUNS] and done.all()
        assert sbr.RUNS == (1, 63, 64, 65, 129)
    if name == "R 1":
        assert np.isnan(table["a_sd"]).all() and (table["a_lo"][done] == table["a_hi"][done]).all() and done.all()
        assert (hist.sum(axis=1) == 1).all()
    if name in ("R 1000", "R 4096"):
        assert (table["replicates"] == R).all() and (table["a_sd"][done] > 0).all()
    if name == "one age":
        assert (table["status"] == 6).all() and (hist[:, 0] == R).all()
    if name == "64 ages":
        assert A == 64
    if name == "level 0.5":
        wide = run(cases()["level 0.999"])
        assert (wide["a_lo"] <= table["a_lo"]).all() and (table["a_hi"] <= wide["a_hi"]).all()
        assert (wide["a_hi"] - wide["a_lo"] > table["a_hi"] - table["a_lo"]).any()
    if name == "70 blocks":
        assert nb.tolist() == [66, 70, 66] and A == 8 and done.all()      # a second batch of draws in every window
    if name == "min_blocks":
        assert case["min_blocks"] == 5 and set(nb.tolist()) == {4, 5}
        assert (table["status"][nb == 4] == 1).all() and (table["status"][nb == 5] != 1).all()
        assert (table["n_failed"][nb == 4] == 0).all() and (table["n_profiles"][nb == 4] > 0).all()
    if name == "a hole":
        empty = table["n_cells"] == 0
        assert empty.sum() >= 2 and (table["status"][empty] == 1).all() and (nb[empty] == 0).all()
        assert np.isnan(table["row"][empty]).all() and not np.isnan(table["t"]).any()
    if name == "a NaN block":
        assert len(table) == 1 and nb[0] == 2 and case["min_blocks"] == 2 and done[0]
        assert table["n_profiles"][0] < table["n_cells"][0]
        assert (ref[0]["terms"][1] == 0).all()                              # the block on NaN ground keeps (0, 0)
        assert table["n_failed"][0] == ref[0]["n_failed"] and 0 < table["n_failed"][0] < R
    if name == "several segments":
        assert sorted(set(table["label"].tolist())) == [2, 5, 9, 11] and (np.diff(table["label"]) >= 0).all()
        one = table[table["label"] == 11]
        assert len(one) == 1 and one["status"][0] == 1 and one["n_blocks"][0] == 1
    # a second run and the run without the histogram: the same bytes
    t2, h2 = run(case, return_hist=True)
    assert t2.tobytes() == table.tobytes() and h2.tobytes() == hist.tobytes()
    assert run(case).tobytes() == table.tobytes()


@pytest.mark.parametrize("name", ["R 1", "a hole", "several segments", "D 3"])
def test_replicate_0_is_fit_along_strike(name):
    """Replicate 0 takes every block once: in every window its index is fit_along_strike's kt_index and its a
    fit_along_strike's a to 1e-9, on the same cells, with and without max_shift.  (The restatement finds no near-tie at
    replicate 0 of these cases.)"""
    case = cases()[name]
    assert not any(r["near"][0] for r in ref_of(name))
    table = run(case)
    o = options(case)
    fit = sl.fit_along_strike(grid(case["z"]), case["cells"], case["labels"], case["angle"], float(case["h"]), float(case["w"]),
                              window=o["window"], step=o["step"], ages=o["ages"], min_samples=o["min_samples"],
                              min_profiles=o["min_profiles"], max_shift=o["max_shift"])
    for f in ("label", "station", "n_cells", "n_profiles", "t", "row", "col"):
        assert fit[f].tobytes() == table[f].tobytes(), f
    done = (table["status"] != 1) & (fit["status"] != 1)
    assert done.sum() >= 3
    assert np.array_equal(table["kt_index0"][done], fit["kt_index"][done])
    assert (np.abs(table["a0"][done] - fit["a"][done]) <= 1e-9 * np.abs(fit["a"][done])).all()
    if case["D"]:
        plain = run(case, max_shift=None)
        assert plain.tobytes() != table.tobytes()
        assert run(case, max_shift=0.0).tobytes() == plain.tobytes()       # D = 0 is the unshifted fit


@pytest.mark.parametrize("name", ["runs", "a NaN block"])
def test_one_window_over_a_segment_is_bootstrap_segments(name):
    """The segments of these cases have one window each, station 0, whose key is bootstrap_segments' and whose blocks are
    the segment's: the integers and the histograms are sl.bootstrap_segments', the floats agree to 1e-9.  (No replicate
    of either restatement lies within a near-tie.)"""
    case = cases()[name]
    table, hist = run(case, return_hist=True)
    seg, hseg = sl.bootstrap_segments(grid(case["z"]), case["cells"], case["labels"], case["angle"], float(case["h"]),
                                      float(case["w"]), block_length=case["block_length"], replicates=case["R"],
                                      level=case["level"], seed=case["seed"], ages=case["ages"],
                                      min_samples=case["min_samples"], min_blocks=case["min_blocks"], return_hist=True)
    assert not any(r["near"].any() for r in ref_of(name))
    assert (table["station"] == 0).all() and len(table) == len(seg)
    for f in ("label", "n_cells", "n_profiles", "n_blocks", "replicates", "n_failed", "kt_index0", "lo_index", "hi_index", "status",
              "kt0", "kt_lo", "kt_hi"):
        assert np.array_equal(table[f], seg[f]), f
    assert np.array_equal(hist, hseg)
    for f in ("a0", "a_mean", "a_sd", "a_lo", "a_hi"):
        assert (np.abs(table[f] - seg[f]) <= 1e-9 * np.abs(seg[f])).all(), f


def test_in_many_chunks_the_same_bytes():
    """The option "fit_chunk" bounds the call's chunks of whole segments and changes no byte: on a context of its own,
    through the binding (the raw rows, padding included), on an uploaded DEM.  The four segments go alone at n = 1, in
    three chunks at n = 72."""
    c = cases()["several segments"]
    a, _ = strike_bootstrap.check_args(c["z"].shape, 1.0, c["cells"], c["labels"], c["angle"], float(c["h"]), float(c["w"]),
                                       c["window"], c["step"], c["block_length"], c["R"], c["level"], c["seed"], c["ages"],
                                       c["min_samples"], c["min_profiles"], c["min_blocks"], None)
    z = np.ascontiguousarray(c["z"], dtype=np.float64)
    sizes = np.diff(a.seg_start)
    assert sizes.tolist() == [40, 60, 71, 1]
    ctx = _lib.Context(0)
    try:
        ctx.profile(0)
        rows, hist = ctx.strike_bootstrap(*a, hist=True, z=z)
        n0 = ctx.profile_get()["k_profile"][0]
        for n, chunks in ((1, 4), (72, 3), (100, 2), (int(sizes.sum()), 1)):
            ctx.set_option("fit_chunk", n)
            try:
                ctx.profile(0)
                got, ghist = ctx.strike_bootstrap(*a, hist=True, z=z)
                launches = ctx.profile_get()["k_profile"][0]
            finally:
                ctx.set_option("fit_chunk", 0)
            assert got.tobytes() == rows.tobytes() and ghist.tobytes() == hist.tobytes(), n
            # the table, then stage one's two launches and the window kernel per chunk
            assert launches == 1 + chunks * (n0 - 1), (n, launches, n0)
        assert n0 == 4
    finally:
        ctx.close()


def test_a_segment_does_not_depend_on_the_others():
    """The rows of a segment are the same bytes whether it is passed alone or with others, and change with its label."""
    case = cases()["several segments"]
    table, hist = run(case, return_hist=True)
    for L in np.unique(table["label"]):
        pick = case["labels"] == L
        t1, h1 = run(case, cells=case["cells"][pick], labels=case["labels"][pick], angle=case["angle"][pick], return_hist=True)
        rows = table["label"] == L
        assert t1.tobytes() == table[rows].tobytes() and h1.tobytes() == hist[rows].tobytes(), L
    pick = case["labels"] == 9
    t9 = table[table["label"] == 9]
    other = run(case, cells=case["cells"][pick], labels=np.full(pick.sum(), 10), angle=case["angle"][pick])
    assert (other["label"] == 10).all() and np.array_equal(other["kt_index0"], t9["kt_index0"])
    assert other["a0"].tobytes() == t9["a0"].tobytes() and other["a_mean"].tobytes() != t9["a_mean"].tobytes()


def test_the_seed_and_the_station_change_the_draws_and_nothing_else():
    case = cases()["R 1000"]
    a = run(case)
    b, hb = run(case, seed=case["seed"] + 1, return_hist=True)
    assert b.tobytes() != a.tobytes() and b["a_mean"].tobytes() != a["a_mean"].tobytes()
    for f in ("label", "station", "n_cells", "n_profiles", "n_blocks", "kt_index0", "a0", "t", "row", "col"):
        assert a[f].tobytes() == b[f].tobytes(), f
    ref = sbr.restate(dict(case, seed=case["seed"] + 1))
    sbr.compare(ref, b, hb)


def test_both_strike_modes_through_the_matcher():
    """A real search, its traces, and the intervals at every station of every segment through the Matcher: the bytes of
    the free function with the same orientations, with strike="cell" and with strike="segment"."""
    g = synthetic.synthetic_scarp(768, theta=0.6)
    m = sl.Matcher(g)
    m.search(sl.Scarp, 100., _plan.age_grid()[::5], _plan.angle_grid())
    res = np.array(m.result_array())
    lo, hi = np.percentile(res[3][res[3] > 0], [60, 90])
    tr = m.extract_traces(lo, hi, 4)
    cells = np.flatnonzero(tr.labels.ravel() > 0)
    assert len(cells) > 50 and len(tr.segments) > 1
    kw = dict(replicates=100, min_blocks=2, seed=11)
    a, ha = m.bootstrap_along_strike(tr, 60., 40., 5., swath=3., return_hist=True, **kw)
    b, hb = sl.bootstrap_along_strike(g, cells, tr.labels, res[2], 60., 3., window=40., block_length=5., return_hist=True, **kw)
    assert a.tobytes() == b.tobytes() and ha.tobytes() == hb.tobytes()
    assert (a["status"] != 1).sum() >= 1 and set(a["label"].tolist()) == set(tr.segments["label"].tolist())
    d = m.bootstrap_along_strike(tr, 60., 40., 5., swath=3., strike="segment", **kw)
    e = sl.bootstrap_along_strike(g, cells, tr.labels, tr.segments["strike"][tr.labels.ravel()[cells] - 1], 60., 3.,
                                  window=40., block_length=5., **kw)
    assert d.tobytes() == e.tobytes() and d.tobytes() != a.tobytes()
    # replicate 0 through the Matcher is the Matcher's fit along the strike
    fit = m.fit_along_strike(tr, 60., 40., swath=3.)
    done = (a["status"] != 1) & (fit["status"] != 1)
    assert np.array_equal(a["station"], fit["station"]) and done.any()
    assert (np.abs(a["a0"][done] - fit["a"][done]) <= 1e-9 * np.abs(fit["a"][done])).all()


def test_the_recovery_case_of_the_docs():
    """docs/strike.md, "Intervals per station": the tapering scarp.  The device counts what the restatement counts - the
    stations, those whose interval holds the planted offset, those whose point estimate lies within 5 % of it."""
    z, cells, planted = sbr.taper_case()
    T = sbr.TAPER
    ages = _plan.age_grid()
    ref = sbr.bootstrap_along_strike(z, 1.0, cells, np.ones(200, dtype=int), 0.0, T["h"], T["w"], ages, T["window"], T["step"],
                                     T["block_length"], T["R"], T["level"], T["seed"], 0, 4, 1, T["min_blocks"])
    table, hist = sl.bootstrap_along_strike(grid(z), cells, np.ones(200, dtype=int), 0.0, float(T["h"]), float(T["w"]),
                                            window=T["window"], step=T["step"], block_length=T["block_length"],
                                            replicates=T["R"], level=T["level"], seed=T["seed"], min_blocks=T["min_blocks"],
                                            return_hist=True)
    sbr.compare(ref, table, hist)
    counts = sbr.taper_counts(table, planted)
    print("stations, intervals that hold the planted offset, point estimates within 5 %%: %s" % (counts,))
    assert counts == sbr.taper_counts(ref, planted)


def test_library_refuses_what_the_header_says():
    """Through the binding, before any device work: what sc_fit_strike refuses, block arrays that do not tile their
    windows exactly, R, level or min_blocks out of range (SC_ERR_INVALID), and a window whose block terms pass 64 KiB
    (SC_ERR_UNSUPPORTED)."""
    import profile_reference as pr
    ctx = _lib.Context(0)
    z = pr.synthetic_z(64)
    i64, i32 = (lambda v: np.array(v, dtype=np.int64)), (lambda v: np.array(v, dtype=np.int32))
    cells, sa, ca = i64([5 * 64 + 30, 6 * 64 + 30, 7 * 64 + 30]), np.zeros(3), np.ones(3)

    def boot(sws=(0, 1, 2), lo=(0, 2), hi=(2, 3), wbs=(0, 2, 3), bhi=(1, 2, 3), D=0, mb=2, R=10, level=0.9, ages=(1.0, 2.0)):
        return ctx.strike_bootstrap(cells, sa, ca, i64([0, 2, 3]), i32([1, 2]), i64(sws), i64(lo), i64(hi), i64(wbs), i64(bhi),
                                    np.array(ages), 10, 1, D, 1.0, 4, 1, mb, R, level, 0, z=z)[0]
    ok = boot()
    assert ok["n_cells"].tolist() == [2, 1] and ok["n_blocks"].tolist() == [2, 1] and ok["status"].tolist()[1] == 1
    assert boot(lo=(1, 3), hi=(1, 3), wbs=(0, 0, 0), bhi=())["n_blocks"].tolist() == [0, 0]     # empty windows are allowed
    for kw in (dict(lo=(0, 1)), dict(sws=(0, 2, 1)), dict(D=-1), dict(D=7),                    # sc_fit_strike's
               dict(bhi=(1, 1, 3)), dict(bhi=(0, 2, 3)), dict(bhi=(1, 3, 3)), dict(bhi=(2, 1, 3)), dict(bhi=(1, 2, 2)),
               dict(wbs=(0, 1, 3)), dict(wbs=(1, 2, 3)), dict(wbs=(0, 2, 2)), dict(wbs=(0, 3, 2)), dict(wbs=(0, 2, 4)),
               dict(R=0), dict(R=4097), dict(level=0.0), dict(level=1.0), dict(level=float("nan")), dict(mb=1)):
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-1\)"):
            boot(**kw)
    # nb A 16 <= 65536: 65 blocks of one cell in one window hold 63 ages and not 64
    n = 65
    zw = pr.synthetic_z(96)
    col = i64(np.arange(10, 10 + n) * 96 + 48)

    def wide(A):
        return ctx.strike_bootstrap(col, np.zeros(n), np.ones(n), i64([0, n]), i32([1]), i64([0, 1]), i64([0]), i64([n]),
                                    i64([0, n]), i64(np.arange(1, n + 1)), 10 ** np.linspace(0, 1.5, A), 10, 1, 0, 1.0, 4, 1, 2,
                                    10, 0.9, 0, z=zw)[0]
    assert wide(63)["n_blocks"].tolist() == [65]
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\)"):
        wide(64)
    ctx.close()
