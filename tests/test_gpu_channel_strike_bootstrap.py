"""sl.bootstrap_channels_along_strike on the MI355X (sc_channel_strike_bootstrap, docs/channels.md "Intervals per station")
against the numpy restatement (tests/channel_strike_bootstrap_reference.py) on the 160 x 160 surfaces of
channel_bootstrap_reference, h = 20, in both depth modes.

Integers - n_blocks, n_profiles, n_failed, the histogram, f_index0, lo_index, hi_index and the status - match the
restatement exactly: the blocks and the draws are integer arithmetic, and a replicate's frequency is an argmin or an argmax
without a subtraction.  The one exception is a window that holds a replicate whose two best keys the restatement finds within
1e-12 relative: such replicates may be at most 0.1 % of a case and none may be replicate 0
(channel_strike_bootstrap_reference.compare asserts it; tests/test_channel_strike_bootstrap_host.py asserts on the CPU that
no case has one).  Floats agree within 1e-9 of their own size, the family's tolerance.  The anchors, the chunks and the
independence of reaches are comparisons with the library's other calls or of bytes."""
import numpy as np
import pytest

import channel_bootstrap_reference as cb
import channel_strike_bootstrap_reference as cwr
import scarplet_amd as sl
from scarplet_amd import _lib, _plan, channel_strike_bootstrap, synthetic

pytestmark = pytest.mark.gpu

NAMES, MODES = cwr.NAMES, cwr.MODES
INTS = ("label", "station", "n_cells", "n_profiles", "n_blocks", "replicates", "n_failed", "f_index0", "lo_index", "hi_index",
        "status")


def case_of(name):
    return cwr.gpu_cases()[NAMES.index(name)]


def ref_of(name, mode):
    """The restatement of a case, computed once (channel_strike_bootstrap_reference keeps it) and left unchanged."""
    return cwr.restate(case_of(name), mode)


def grid(case):
    return sl.DEMGrid.from_array(case["z"], case["de"])


def options(case, mode, **kw):
    args = dict(swath=float(case["w"]), window=case["window"], step=case["step"], block_length=case["block_length"],
                max_shift=float(case["D"]), depth=mode, replicates=case["R"], level=case["level"], seed=case["seed"],
                min_samples=case["min_samples"], min_profiles=case["min_profiles"], min_blocks=case["min_blocks"])
    args.update(kw)
    return args


def run(case, mode, cells=None, labels=None, angle=None, **kw):
    return sl.bootstrap_channels_along_strike(grid(case), case["cells"] if cells is None else cells,
                                              case["labels"] if labels is None else labels,
                                              case["angle"] if angle is None else angle, float(case["h"]), case["frequencies"],
                                              **options(case, mode, **kw))


def test_the_case_list_is_the_one_named_here():
    cases = cwr.gpu_cases()
    assert [c["name"] for c in cases] == NAMES
    for c in cases:
        assert c["z"].shape == (160, 160) and c["h"] == 20 and len(c["cells"]) <= 300


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_against_the_restatement(name, mode):
    case = case_of(name)
    table, hist = run(case, mode, return_hist=True)
    ref = ref_of(name, mode)
    F, R = len(case["frequencies"]), case["R"]
    assert len(table) == len(ref) and hist.shape == (len(ref), F) and hist.dtype == np.int32
    st = cwr.compare(ref, table, hist)
    print("%s, %s: %s" % (name, mode, st))
    done = table["status"] & 1 == 0
    assert done.any()
    i0 = table["f_index0"]
    assert np.array_equal(table["f0"][done & (i0 >= 0)], case["frequencies"][i0[done & (i0 >= 0)]])
    assert np.array_equal(table["f_lo"][done], case["frequencies"][table["lo_index"][done]])
    assert np.array_equal(table["f_hi"][done], case["frequencies"][table["hi_index"][done]])
    assert (hist.sum(axis=1)[done] == R - table["n_failed"][done]).all() and not hist[~done].any()
    nb = table["n_blocks"]
    if name == "nb 1 4 5 70":
        assert table["label"].tolist() == [2, 4, 6, 9] and nb.tolist() == [4, 70, 1, 5] and case["min_blocks"] == 5
        assert done.tolist() == [False, True, False, True] and (table["station"] == 0).all()
    if name == "R 1":
        assert np.isnan(table["a_sd"]).all() and (table["a_lo"][done] == table["a_hi"][done]).all()
        assert (hist.sum(axis=1)[done] == 1).all() and (table["area_lo"][done] == table["area_hi"][done]).all()
    if name in ("R 1000", "R 4096"):
        assert (table["replicates"] == R).all() and (table["a_sd"][done] > 0).all() and (table["area_sd"][done] > 0).all()
    if name == "F 1":
        assert (table["status"][done] == 6).all() and (hist[done, 0] == R).all()
    if name == "level 0.5":
        wide = run(case_of("level 0.999"), mode)
        assert (wide["a_lo"][done] <= table["a_lo"][done]).all() and (table["a_hi"][done] <= wide["a_hi"][done]).all()
        assert (wide["a_hi"] - wide["a_lo"] > table["a_hi"] - table["a_lo"])[done].any()
    if name.startswith("run"):
        assert (nb == 2).all() and done.all() and table["n_profiles"].tolist() == [int(c) + 3 for c in name.split()[1:]]
    if name == "an empty block":
        assert any((r["mb"] == 0).any() and r["status"] & 1 == 0 for r in ref)
    if name == "empty windows":
        empty = table["n_cells"] == 0
        assert empty.sum() >= 2 and (table["status"][empty] == 1).all() and (nb[empty] == 0).all()
        assert np.isnan(table["row"][empty]).all() and not np.isnan(table["t"]).any()
        blind = (table["n_cells"] > 0) & (table["n_profiles"] == 0)
        assert blind.any() and (table["status"][blind] == 1).all() and (nb[blind] > 0).all()
    if name == "a dead frequency":
        # the last frequency is dead in replicate 0 and in the replicates that draw the third block, live in the others
        assert len(table) == 1 and len(set(ref[0]["n_live"].tolist())) == 2 and ref[0]["n_live"][0] == F - 1
    if name == "no live frequency":
        assert table["status"].tolist() == [33, 6, 6] and table["n_failed"][0] == R and 0 < table["n_failed"][2] < R
        assert table["n_profiles"].tolist() == [30, 30, 30] and np.isnan(table["f0"][2]) and table["f_index0"][2] == -1
    if name == "several reaches":
        assert sorted(set(table["label"].tolist())) == [2, 4, 9, 11, 12] and (np.diff(table["label"]) >= 0).all()
        assert np.any(np.diff(case["labels"]) < 0)
        for L in (11, 12):
            one = table[table["label"] == L]
            assert len(one) == 1 and one["status"][0] == 1 and one["n_blocks"][0] == 1 and one["n_cells"][0] == 1
    if name == "caps":
        assert R == 4096 and F == 64 and nb.max() == 64 and 16 * 64 * F == _lib.CHANNEL_STRIKE_BOOT_LDS_TERMS
    # a second run and the run without the histogram: the same bytes
    t2, h2 = run(case, mode, return_hist=True)
    assert t2.tobytes() == table.tobytes() and h2.tobytes() == hist.tobytes()
    assert run(case, mode).tobytes() == table.tobytes()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["R 1", "an empty block", "several reaches", "D 3"])
def test_replicate_0_is_fit_channels_along_strike(name, mode):
    """Replicate 0 takes every block once: in every window its index is fit_channels_along_strike's f_index and its a that
    call's a to 1e-9, on the same cells, with and without max_shift.  (The restatement finds no near-tie at replicate 0.)"""
    case = case_of(name)
    assert not any(r["near"][0] for r in ref_of(name, mode))
    table = run(case, mode)
    o = options(case, mode)
    fit = sl.fit_channels_along_strike(grid(case), case["cells"], case["labels"], case["angle"], float(case["h"]),
                                       case["frequencies"], swath=o["swath"], window=o["window"], step=o["step"],
                                       max_shift=o["max_shift"], depth=mode, min_samples=o["min_samples"],
                                       min_profiles=o["min_profiles"])
    for f in ("label", "station", "n_cells", "n_profiles", "t", "row", "col"):
        assert fit[f].tobytes() == table[f].tobytes(), f
    done = (table["status"] & 1 == 0) & (fit["status"] & 1 == 0)
    assert done.sum() >= 3
    assert np.array_equal(table["f_index0"][done], fit["f_index"][done])
    assert (np.abs(table["a0"][done] - fit["a"][done]) <= 1e-9 * np.abs(fit["a"][done])).all()
    if case["D"]:
        plain = run(case, mode, max_shift=0.0)
        assert plain.tobytes() != table.tobytes()
        fit0 = sl.fit_channels_along_strike(grid(case), case["cells"], case["labels"], case["angle"], float(case["h"]),
                                            case["frequencies"], swath=o["swath"], window=o["window"], step=o["step"],
                                            depth=mode, min_samples=o["min_samples"])
        assert np.array_equal(plain["f_index0"][done], fit0["f_index"][done])
        assert (np.abs(plain["a0"][done] - fit0["a"][done]) <= 1e-9 * np.abs(fit0["a"][done])).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["nb 1 4 5 70", "runs 63 64 65", "a dead frequency", "no live frequency"])
def test_one_window_over_a_reach_is_bootstrap_channel_segments(name, mode):
    """The reaches of these cases have one window each, station 0, whose key is bootstrap_channel_segments' and whose blocks
    are the reach's: the integers and the histograms are sl.bootstrap_channel_segments', the floats agree to 1e-9 (the
    profiles of a block are added in another order).  (No replicate of either restatement lies within a near-tie.)"""
    case = case_of(name)
    table, hist = run(case, mode, return_hist=True)
    seg, hseg = sl.bootstrap_channel_segments(grid(case), case["cells"], case["labels"], case["angle"], float(case["h"]),
                                              case["frequencies"], swath=float(case["w"]), max_shift=float(case["D"]), depth=mode,
                                              block_length=case["block_length"], replicates=case["R"], level=case["level"],
                                              seed=case["seed"], min_samples=case["min_samples"],
                                              min_profiles=case["min_profiles"], min_blocks=case["min_blocks"], return_hist=True)
    assert not any(r["near"].any() for r in ref_of(name, mode))
    assert not any(r["near"].any() for r in cb.restate(dict(case, name="one window, " + name), mode))
    assert (table["station"] == 0).all() and len(table) == len(seg)
    for f in INTS:
        if f != "station":
            assert np.array_equal(table[f], seg[f]), f
    for f in ("f0", "f_lo", "f_hi"):
        assert np.array_equal(table[f], seg[f], equal_nan=True), f
    assert np.array_equal(hist, hseg)
    for f in cb.ROW_FLOATS[3:] + cb.DERIVED:
        ok = ~np.isnan(seg[f])
        assert np.array_equal(np.isnan(table[f]), ~ok), f
        assert (np.abs(table[f][ok] - seg[f][ok]) <= 1e-9 * np.abs(seg[f][ok])).all(), f


@pytest.mark.parametrize("mode", MODES)
def test_in_many_chunks_the_same_bytes(mode):
    """The option "fit_chunk" bounds the call's chunks of whole reaches and changes no byte: on a context of its own, through
    the binding (the raw rows, padding included), on an uploaded DEM.  The five reaches go alone at n = 1, in several chunks
    at n = 8 and 104, in one at their sum."""
    c = case_of("several reaches")
    a, _ = channel_strike_bootstrap.check_args(c["z"].shape, c["de"], c["cells"], c["labels"], c["angle"], float(c["h"]),
                                               c["frequencies"], float(c["w"]), c["window"], c["step"], c["block_length"],
                                               float(c["D"]), mode, c["R"], c["level"], c["seed"], c["min_samples"],
                                               c["min_profiles"], c["min_blocks"])
    z = np.ascontiguousarray(c["z"], dtype=np.float64)
    sizes = np.diff(a.seg_start)
    assert sizes.tolist() == [6, 103, 7, 1, 1]
    ctx = _lib.Context(0)
    try:
        ctx.profile(0)
        rows, hist = ctx.channel_strike_bootstrap(*a, hist=True, z=z)
        n0 = ctx.profile_get()["k_profile"][0]
        for n, chunks in ((1, 5), (8, 4), (104, 3), (110, 2), (int(sizes.sum()), 1)):
            ctx.set_option("fit_chunk", n)
            try:
                ctx.profile(0)
                got, ghist = ctx.channel_strike_bootstrap(*a, hist=True, z=z)
                launches = ctx.profile_get()["k_profile"][0]
            finally:
                ctx.set_option("fit_chunk", 0)
            assert got.tobytes() == rows.tobytes() and ghist.tobytes() == hist.tobytes(), n
            # the tables once, then stage one's two launches and the window kernel per chunk
            assert launches == (n0 - 3) + 3 * chunks, (n, launches, n0)
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", MODES)
def test_a_reach_does_not_depend_on_the_others(mode):
    """The rows of a reach are the same bytes whether it is passed alone or with others, and change with its label."""
    case = case_of("several reaches")
    table, hist = run(case, mode, return_hist=True)
    for L in np.unique(table["label"]):
        pick = case["labels"] == L
        t1, h1 = run(case, mode, cells=case["cells"][pick], labels=case["labels"][pick], angle=case["angle"][pick],
                     return_hist=True)
        rows = table["label"] == L
        assert t1.tobytes() == table[rows].tobytes() and h1.tobytes() == hist[rows].tobytes(), L
    pick = case["labels"] == 4
    t4 = table[table["label"] == 4]
    other = run(case, mode, cells=case["cells"][pick], labels=np.full(pick.sum(), 10), angle=case["angle"][pick])
    assert (other["label"] == 10).all() and np.array_equal(other["f_index0"], t4["f_index0"])
    assert other["a0"].tobytes() == t4["a0"].tobytes() and other["a_mean"].tobytes() != t4["a_mean"].tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_the_seed_changes_the_draws_and_nothing_else(mode):
    case = case_of("R 1000")
    a = run(case, mode)
    b, hb = run(case, mode, seed=case["seed"] + 1, return_hist=True)
    assert b.tobytes() != a.tobytes() and b["a_mean"].tobytes() != a["a_mean"].tobytes()
    for f in ("label", "station", "n_cells", "n_profiles", "n_blocks", "f_index0", "a0", "area0", "t", "row", "col"):
        assert a[f].tobytes() == b[f].tobytes(), f
    cwr.compare(cwr.restate(dict(case, seed=case["seed"] + 1), mode), b, hb)


@pytest.mark.parametrize("mode", MODES)
def test_the_same_window_at_another_station_has_other_draws(mode):
    """The station is in the key.  Thirty cells of one column at orientation 0 (t = row) in windows of 10 every 5: without
    the cells of the first five rows the reach is one step shorter, its stations lie where stations 1, 2, ... lay, and the
    windows that hold none of the dropped rows hold the same cells in the same blocks under a station number one lower.
    What no draw decides - the counts, replicate 0 - is the same bytes; what the draws decide is not, and is the
    restatement's with that station in the key."""
    full = dict(case_of("a dead frequency"), window=10.0, step=5.0, block_length=2.0, min_blocks=3)
    assert (full["angle"] == 0.0).all() and (np.diff(np.sort(full["cells"] // 160)) == 1).all()
    keep = full["cells"] // 160 >= (full["cells"] // 160).min() + 5
    cut = dict(full, name="a dead frequency, five rows shorter", stage="dead cut", cells=full["cells"][keep],
               labels=full["labels"][keep], angle=full["angle"][keep])
    a, ha = run(full, mode, return_hist=True)
    b, hb = run(cut, mode, return_hist=True)
    assert len(a) == len(b) + 1
    same = [k for k in range(len(b)) if a["n_cells"][k + 1] == b["n_cells"][k] and a["row"][k + 1] == b["row"][k]
            and a["t"][k + 1] == b["t"][k] and b["status"][k] & 1 == 0]
    assert len(same) >= 3
    k = np.array(same)
    assert (a["station"][k + 1] == b["station"][k] + 1).all()
    for f in ("label", "n_cells", "n_profiles", "n_blocks", "replicates", "f_index0", "f0", "a0", "area0", "t", "row", "col"):
        assert a[f][k + 1].tobytes() == b[f][k].tobytes(), f
    # (most replicates of these windows choose one frequency, so a histogram may agree by chance; the means do not)
    assert all(a["a_mean"][i + 1] != b["a_mean"][i] and a["a_sd"][i + 1] != b["a_sd"][i] for i in same)
    assert any(ha[i + 1].tobytes() != hb[i].tobytes() for i in same)
    cwr.compare(cwr.restate(cut, mode), b, hb)


def test_both_strike_modes_through_the_matcher():
    """A real search, its traces, and the intervals at every station of every segment through the Matcher: the bytes of the
    free function with the same orientations, with strike="cell" and with strike="segment"."""
    g = synthetic.synthetic_scarp(768, theta=0.6)
    m = sl.Matcher(g)
    m.search(sl.Scarp, 100., _plan.age_grid()[::5], _plan.angle_grid())
    res = np.array(m.result_array())
    lo, hi = np.percentile(res[3][res[3] > 0], [60, 90])
    tr = m.extract_traces(lo, hi, 4)
    cells = np.flatnonzero(tr.labels.ravel() > 0)
    assert len(cells) > 50 and len(tr.segments) > 1
    fs = cb.FS8
    kw = dict(replicates=100, min_blocks=2, seed=11, depth="segment")
    a, ha = m.bootstrap_channels_along_strike(tr, 20., fs, 40., 5., swath=1., return_hist=True, **kw)
    b, hb = sl.bootstrap_channels_along_strike(g, cells, tr.labels, res[2], 20., fs, 1., window=40., block_length=5.,
                                               return_hist=True, **kw)
    assert a.tobytes() == b.tobytes() and ha.tobytes() == hb.tobytes()
    assert set(a["label"].tolist()) == set(tr.segments["label"].tolist()) and (a["n_blocks"] >= 2).any()
    d = m.bootstrap_channels_along_strike(tr, 20., fs, 40., 5., swath=1., strike="segment", **kw)
    e = sl.bootstrap_channels_along_strike(g, cells, tr.labels, tr.segments["strike"][tr.labels.ravel()[cells] - 1], 20., fs, 1.,
                                           window=40., block_length=5., **kw)
    assert d.tobytes() == e.tobytes() and d.tobytes() != a.tobytes()
    # the stations are the Matcher's fit along the strike
    fit = m.fit_channels_along_strike(tr, 20., fs, 40., swath=1., depth="segment")
    for f in ("label", "station", "n_cells", "n_profiles", "t"):
        assert fit[f].tobytes() == a[f].tobytes(), f


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("span", cwr.REC_SPANS)
def test_the_recovery_table_of_the_docs(span, mode):
    """docs/channels.md, "Intervals per station": the widening trough (span 3) and the trough of constant width (span 0) in
    windows of 60 every 30 and blocks of 9.  The device returns the restatement's table, which is the docs'
    (channel_strike_bootstrap_reference.REC_INTERVALS; tests/test_channel_strike_bootstrap_host.py pins the restatement to
    it)."""
    case = cwr.recovery(span)
    ref = cwr.restate(case, mode)
    table, hist = run(case, mode, return_hist=True)
    print("span %d, %s: %s" % (span, mode, cwr.compare(ref, table, hist)))
    got = [[int(r["lo_index"]), int(r["hi_index"])] for r in table]
    assert got == [[r["lo_index"], r["hi_index"]] for r in ref] == cwr.REC_INTERVALS[span]
    assert (table["status"] & 1 == 0).all() and len(table) == 11


def test_library_refuses_what_the_header_says():
    """Through the binding, before any device work: what sc_channel_strike refuses, block arrays that do not tile their
    windows exactly, R, level or min_blocks out of range (SC_ERR_INVALID), and a window whose block terms pass 64 KiB or more
    than 64 frequencies (SC_ERR_UNSUPPORTED)."""
    ctx = _lib.Context(0)
    z = cb.gpu_cases()[0]["z"][:64, :64].copy()
    i64, i32 = (lambda v: np.array(v, dtype=np.int64)), (lambda v: np.array(v, dtype=np.int32))
    cells, sa, ca = i64([25 * 64 + 30, 26 * 64 + 30, 27 * 64 + 30]), np.zeros(3), np.ones(3)

    def boot(sws=(0, 1, 2), lo=(0, 2), hi=(2, 3), wbs=(0, 2, 3), bhi=(1, 2, 3), D=0, mode=0, mb=2, R=10, level=0.9,
             fs=(0.05, 0.1), de=1.0):
        return ctx.channel_strike_bootstrap(cells, sa, ca, i64([0, 2, 3]), i32([1, 2]), i64(sws), i64(lo), i64(hi), i64(wbs),
                                            i64(bhi), np.array(fs), 10, 1, D, mode, de, 4, 1, mb, R, level, 0, z=z)[0]
    ok = boot()
    assert ok["n_cells"].tolist() == [2, 1] and ok["n_blocks"].tolist() == [2, 1] and ok["status"].tolist()[1] == 1
    assert ok["status"][0] & 1 == 0 and boot(mode=1)["status"][0] & 1 == 0
    assert boot(lo=(1, 3), hi=(1, 3), wbs=(0, 0, 0), bhi=())["n_blocks"].tolist() == [0, 0]     # empty windows are allowed
    for kw in (dict(lo=(0, 1)), dict(sws=(0, 2, 1)), dict(D=-1), dict(D=7), dict(mode=2), dict(mode=-1),     # sc_channel_strike's
               dict(fs=(0.1, 0.05)), dict(fs=(0.0, 0.1)), dict(fs=(0.05, 2.0)), dict(de=0.0),
               dict(bhi=(1, 1, 3)), dict(bhi=(0, 2, 3)), dict(bhi=(1, 3, 3)), dict(bhi=(2, 1, 3)), dict(bhi=(1, 2, 2)),
               dict(wbs=(0, 1, 3)), dict(wbs=(1, 2, 3)), dict(wbs=(0, 2, 2)), dict(wbs=(0, 3, 2)), dict(wbs=(0, 2, 4)),
               dict(R=0), dict(R=4097), dict(level=0.0), dict(level=1.0), dict(level=float("nan")), dict(mb=1)):
        with pytest.raises(_lib.ScarpletHipError, match=r"\(-1\)"):
            boot(**kw)
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\)"):
        boot(fs=np.linspace(0.01, 0.1, 65))
    # nb F 16 <= 65536: 65 blocks of one cell in one window hold 63 frequencies and not 64
    n = 65
    zw = cb.gpu_cases()[0]["z"][:96, :96].copy()
    col = i64(np.arange(10, 10 + n) * 96 + 48)

    def wide(F):
        return ctx.channel_strike_bootstrap(col, np.zeros(n), np.ones(n), i64([0, n]), i32([1]), i64([0, 1]), i64([0]), i64([n]),
                                            i64([0, n]), i64(np.arange(1, n + 1)), np.geomspace(0.01, 0.2, F), 10, 1, 0, 0, 1.0, 4,
                                            1, 2, 10, 0.9, 0, z=zw)[0]
    assert wide(63)["n_blocks"].tolist() == [65]
    with pytest.raises(_lib.ScarpletHipError, match=r"\(-4\)"):
        wide(64)
    ctx.close()
