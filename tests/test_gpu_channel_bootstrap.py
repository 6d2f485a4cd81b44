"""sl.bootstrap_channel_segments on the MI355X (sc_channel_bootstrap; docs/channels.md, "Intervals per reach") against the numpy
restatement (tests/channel_bootstrap_reference.py), in both depth modes, on 160 x 160 DEMs at h = 20.

Integers - n_blocks, n_profiles, n_failed, every replicate's index, the histogram, lo_index and hi_index - match the
restatement exactly: the draws are integer arithmetic and a replicate's frequency is an argmax or an argmin without a
subtraction.  The one exception is a replicate whose two best keys the restatement finds within 1e-12 relative: such
replicates may be at most 0.1 % of a case (channel_bootstrap_reference.compare asserts it on the restatement alone;
tests/test_channel_bootstrap_host.py shows that the cases hold none at replicate 0).  Floats, the standard deviations
included, agree within the family's 1e-9 of their own size - the restatement agrees with its longdouble twin within 1e-11 on
every input here.  The anchors are byte comparisons."""
import contextlib

import numpy as np
import pytest

import channel_bootstrap_reference as cb
import scarplet_amd as sl
from scarplet_amd import core, synthetic

pytestmark = pytest.mark.gpu

NAMES = ["nb 1 4 5 70", "R 1", "R 1000", "F 1", "F 64", "D 3", "a block of 130", "an empty block", "clipped by the edge",
         "a dead frequency", "no live frequency", "R 4096, F 64"]
ALL = dict(return_hist=True, return_replicates=True)


def case_of(name):
    return cb.gpu_cases()[NAMES.index(name)]


def grid(z, de=1.0):
    return sl.DEMGrid.from_array(z, float(de))


def run(case, mode, cells=None, labels=None, angle=None, **kw):
    de = case["de"]
    args = dict(swath=case["w"] * de, max_shift=case["D"] * de, depth=mode, block_length=case["block_length"],
                replicates=case["R"], level=case["level"], seed=case["seed"], min_samples=case["min_samples"],
                min_profiles=case["min_profiles"], min_blocks=case["min_blocks"])
    args.update(kw)
    return sl.bootstrap_channel_segments(grid(case["z"], de), case["cells"] if cells is None else cells,
                                         case["labels"] if labels is None else labels, case["angle"] if angle is None else angle,
                                         case["h"] * de, case["frequencies"], **args)


def fit(case, mode, **kw):
    de = case["de"]
    args = dict(swath=case["w"] * de, max_shift=case["D"] * de, depth=mode, min_samples=case["min_samples"],
                min_profiles=case["min_profiles"])
    args.update(kw)
    return sl.fit_channel_segments(grid(case["z"], de), case["cells"], case["labels"], case["angle"], case["h"] * de,
                                   case["frequencies"], **args)


def same_bytes(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


@contextlib.contextmanager
def option(name, value, default):
    ctx = core._context(0)
    ctx.set_option(name, value)
    try:
        yield ctx
    finally:
        ctx.set_option(name, default)


def test_the_case_list_is_the_one_named_here():
    assert [c["name"] for c in cb.gpu_cases()] == NAMES == cb.NAMES
    for c in cb.gpu_cases():
        assert max(c["z"].shape) <= 160 and c["h"] <= 20 and len(c["cells"]) <= 300


# ---- 1. against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", cb.MODES)
@pytest.mark.parametrize("name", NAMES)
def test_against_the_restatement(name, mode):
    case = case_of(name)
    fs = case["frequencies"]
    table, hist, index, amp = run(case, mode, **ALL)
    S, F, R = len(np.unique(case["labels"][case["labels"] > 0])), len(fs), case["R"]
    assert len(table) == S and hist.shape == (S, F) and hist.dtype == np.int32
    assert index.shape == (S, R + 1) and index.dtype == np.int8 and amp.shape == (S, R + 1) and amp.dtype == np.float64
    ref = cb.restate(case, mode)
    st = cb.compare(ref, table, hist, index, amp, fs)
    print("%s, %s: %s" % (name, mode, st))
    done = table["status"] & 1 == 0
    assert np.array_equal(table["f_lo"][done], fs[table["lo_index"][done]])
    assert np.array_equal(table["f_hi"][done], fs[table["hi_index"][done]])
    assert np.array_equal(index[done, 0], table["f_index0"][done])
    assert (hist.sum(axis=1) == np.where(done, R - table["n_failed"], 0)).all()
    by = {int(r["label"]): r for r in table}
    if name in ("nb 1 4 5 70", "R 1", "R 1000", "F 1", "F 64", "D 3", "R 4096, F 64"):
        # 1 and 4 blocks against min_blocks = 5: status 1; 5 blocks; 70: more than one round of 64 draws
        assert table["n_blocks"].tolist() == [4, 70, 1, 5] and case["min_blocks"] == 5
        assert table["status"][[0, 2]].tolist() == [1, 1] and done[[1, 3]].all()
    if name == "F 1":
        assert (table["status"][[1, 3]] == 6).all() and (index[[1, 3]] == 0).all()
    if name in ("F 64", "R 4096, F 64"):
        # the terms of the 70 blocks leave the LDS, those of the 5 fit
        assert 70 * F * 16 > 65536 >= 5 * F * 16
    if name == "R 1":
        assert np.isnan(table["a_sd"]).all() and np.isnan(table["area_sd"]).all() and (table["a_lo"][done] == table["a_hi"][done]).all()
    if name == "a block of 130":
        assert ref[0]["mb"].max() > 130 and table["n_profiles"][0] == 300
    if name == "an empty block":
        assert (ref[0]["mb"] == 0).any() and table["n_blocks"][0] == len(ref[0]["mb"]) and done[0]
        assert table["n_profiles"][0] < table["n_cells"][0]
    if name == "clipped by the edge":
        assert 0 < table["n_profiles"][0] < table["n_cells"][0] and done[0]
    if name == "a dead frequency":
        # the narrowest frequency is dead in the third block alone: replicate 0 does not count it, the replicates that miss the
        # block choose it, and no replicate fails
        miss = ~(ref[0]["picks"] == 2).any(axis=1)
        assert 0 <= index[0, 0] < F - 1 and np.array_equal(index[0] == F - 1, miss) and table["n_failed"][0] == 0
        assert hist[0, F - 1] == miss[1:].sum() > 0 and (index[0] >= 0).all()
    if name == "no live frequency":
        assert table["status"].tolist() == [33, 6, 6] and table["n_failed"].tolist() == [R, 0, int((index[2, 1:] < 0).sum())]
        assert by[3]["f_index0"] == -1 and np.isnan(by[3]["a0"]) and np.isnan(by[3]["area0"]) and 0 < by[3]["n_failed"] < R
    # a second run and the runs without the optional outputs: the same bytes
    same_bytes(run(case, mode, **ALL), (table, hist, index, amp))
    assert run(case, mode).tobytes() == table.tobytes()
    same_bytes(run(case, mode, return_hist=True), (table, hist))
    same_bytes(run(case, mode, return_replicates=True), (table, index, amp))


# ---- 2. anchors -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", cb.MODES)
@pytest.mark.parametrize("name", ["nb 1 4 5 70", "D 3", "a block of 130", "an empty block", "a dead frequency"])
def test_replicate_0_is_fit_channel_segments(name, mode):
    """Replicate 0 takes every block once: its index is fit_channel_segments' f_index and its a that call's a to 1e-9, on the
    same cells, with and without max_shift.  (The restatement finds no near-tie at replicate 0 of these cases.)"""
    case = case_of(name)
    assert not any(r["near"][0] for r in cb.restate(case, mode))
    table = run(case, mode)
    pooled = fit(case, mode)
    assert np.array_equal(pooled["label"], table["label"]) and np.array_equal(pooled["n_profiles"], table["n_profiles"])
    assert np.array_equal(pooled["n_cells"], table["n_cells"])
    done = table["status"] & 1 == 0
    assert done.any() and (pooled["status"][done] & 1 == 0).all()
    assert np.array_equal(table["f_index0"][done], pooled["f_index"][done])
    assert (np.abs(table["a0"][done] - pooled["a"][done]) <= 1e-9 * np.abs(pooled["a"][done])).all()
    assert (np.abs(table["area0"][done] - pooled["area"][done]) <= 1e-9 * np.abs(pooled["area"][done])).all()
    if case["D"]:
        plain = run(dict(case, D=0), mode)
        assert plain.tobytes() != table.tobytes()
    else:
        # max_shift = 0 is the call without a shift: the default, left out here, and a range below one cell return its bytes
        de = case["de"]
        plain = sl.bootstrap_channel_segments(grid(case["z"], de), case["cells"], case["labels"], case["angle"], case["h"] * de,
                                              case["frequencies"], swath=case["w"] * de, depth=mode,
                                              block_length=case["block_length"], replicates=case["R"], level=case["level"],
                                              seed=case["seed"], min_samples=case["min_samples"],
                                              min_profiles=case["min_profiles"], min_blocks=case["min_blocks"])
        assert plain.tobytes() == table.tobytes() == run(case, mode, max_shift=0.5 * de).tobytes()


@pytest.mark.parametrize("mode", cb.MODES)
def test_a_reach_does_not_depend_on_the_others(mode):
    """The rows of a reach are the same bytes whether it is passed alone or with others, in one chunk or in several, and a
    changed label changes the draws and nothing else."""
    case = case_of("nb 1 4 5 70")
    table, hist, index, amp = run(case, mode, **ALL)
    for s, L in enumerate(table["label"]):
        pick = case["labels"] == L
        one = run(case, mode, cells=case["cells"][pick], labels=case["labels"][pick], angle=case["angle"][pick], **ALL)
        same_bytes(one, (table[s:s + 1], hist[s:s + 1], index[s:s + 1], amp[s:s + 1]))
    for n in (1, 70):
        with option("fit_chunk", n, 0):
            same_bytes(run(case, mode, **ALL), (table, hist, index, amp))
    with option("channel_terms", 0, 1):
        same_bytes(run(case, mode, **ALL), (table, hist, index, amp))
    pick = case["labels"] == 4
    t5, i5, a5 = run(case, mode, cells=case["cells"][pick], labels=np.full(pick.sum(), 5), angle=case["angle"][pick],
                     return_replicates=True)
    assert t5["label"][0] == 5 and a5[0, 1:].tobytes() != amp[1, 1:].tobytes()
    for f in ("n_cells", "n_profiles", "n_blocks", "replicates", "f_index0", "f0", "a0", "area0"):
        assert t5[f][0] == table[f][1], f
    assert i5[0, 0] == index[1, 0] and a5[0, 0] == amp[1, 0]
    ref = cb.restate(dict(case, name="nb 70 as label 5", cells=case["cells"][pick], labels=np.full(pick.sum(), 5),
                          angle=case["angle"][pick], stage="nb 70 as label 5"), mode)
    _, h5, i5, a5 = run(case, mode, cells=case["cells"][pick], labels=np.full(pick.sum(), 5), angle=case["angle"][pick], **ALL)
    cb.compare(ref, t5, h5, i5, a5, case["frequencies"])


@pytest.mark.parametrize("mode", cb.MODES)
def test_the_seed_changes_the_draws_and_nothing_else(mode):
    case = case_of("nb 1 4 5 70")
    a, ia, aa = run(case, mode, return_replicates=True)
    b, hb, ib, ab = run(case, mode, seed=case["seed"] + 1, **ALL)
    assert b.tobytes() != a.tobytes() and ab[:, 1:].tobytes() != aa[:, 1:].tobytes()
    assert np.array_equal(ib[:, 0], ia[:, 0]) and ab[:, 0].tobytes() == aa[:, 0].tobytes()
    for f in ("label", "n_cells", "n_profiles", "n_blocks", "replicates", "f_index0", "f0", "a0", "area0"):
        assert a[f].tobytes() == b[f].tobytes(), f
    ref = cb.restate(dict(case, name="nb 1 4 5 70, seed + 1", seed=case["seed"] + 1), mode)
    cb.compare(ref, b, hb, ib, ab, case["frequencies"])


def test_both_strike_modes_through_the_matcher():
    """A Channel search, its traces, and the bootstrap of every segment through the Matcher: the bytes of the free function
    with the same orientations, with strike="cell" and with strike="segment"."""
    g = synthetic.synthetic_channel(512)
    m = sl.Matcher(g)
    f0 = 0.035
    m.search(sl.Channel, 50.0, [f0], np.linspace(-0.3, 0.3, 9))
    res = np.array(m.result_array())
    top = float(np.nanmax(res[3]))
    tr = m.extract_traces(0.25 * top, 0.5 * top, 4)
    cells = np.flatnonzero(tr.labels.ravel() > 0)
    assert len(cells) > 50 and len(tr.segments) >= 1
    fs = f0 * 1.12 ** np.arange(-6, 7)
    for mode in cb.MODES:
        kw = dict(swath=2.0, max_shift=3.0, depth=mode, replicates=100, min_blocks=2, seed=11, **ALL)
        a = m.bootstrap_channel_segments(tr, 30.0, fs, 8.0, **kw)
        b = sl.bootstrap_channel_segments(g, cells, tr.labels, res[2], 30.0, fs, block_length=8.0, **kw)
        same_bytes(a, b)
        assert np.array_equal(a[0]["label"], tr.segments["label"]) and np.array_equal(a[0]["n_cells"], tr.segments["n_cells"])
        assert (a[0]["status"] & 1 == 0).any()
        d = m.bootstrap_channel_segments(tr, 30.0, fs, 8.0, strike="segment", **kw)
        e = sl.bootstrap_channel_segments(g, cells, tr.labels, tr.segments["strike"][tr.labels.ravel()[cells] - 1], 30.0, fs,
                                          block_length=8.0, **kw)
        same_bytes(d, e)
        assert d[0].tobytes() != a[0].tobytes()
        # replicate 0 through the Matcher is the Matcher's joint fit
        pooled = m.fit_channel_segments(tr, 30.0, fs, swath=2.0, max_shift=3.0, depth=mode)
        done = a[0]["status"] & 1 == 0
        assert np.array_equal(a[0]["f_index0"][done], pooled["f_index"][done])
        assert (np.abs(a[0]["a0"][done] - pooled["a"][done]) <= 1e-9 * np.abs(pooled["a"][done])).all()
    # the search's record is what it was
    assert np.array_equal(np.array(m.result_array()), res, equal_nan=True)


# ---- 3. the widening trough -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", cb.MODES)
@pytest.mark.parametrize("span", cb.WIDE_SPANS)
def test_the_widening_trough_is_the_restatements(span, mode):
    """docs/channels.md, "Intervals per reach": the device's intervals and histograms on the reach of one width and on the
    reach that widens by a factor of 2 are the restatement's; fit_channel_segments' interval is one frequency wide on both."""
    case = cb.widening_case(span)
    table, hist, index, amp = run(case, mode, **ALL)
    ref = cb.restate(case, mode)
    st = cb.compare(ref, table, hist, index, amp, case["frequencies"])
    print("span %g, %s: %s" % (span, mode, st))
    first, counts = cb.WIDE_HIST[(span, mode)]
    want = np.zeros(len(case["frequencies"]), dtype=np.int32)
    want[first:first + len(counts)] = counts
    assert np.array_equal(hist[0], want) and np.array_equal(hist[0], ref[0]["hist"])
    pooled = fit(case, mode)
    assert pooled["lo_index"][0] == pooled["hi_index"][0] == pooled["f_index"][0] == table["f_index0"][0] == 13
    got = (int(table["lo_index"][0]), int(table["hi_index"][0]))
    assert got == ((13, 13) if span == 0 else (12, 14)) == (ref[0]["lo_index"], ref[0]["hi_index"])
