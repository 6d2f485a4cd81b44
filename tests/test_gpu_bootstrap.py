"""sl.bootstrap_segments on the MI355X (sc_bootstrap_segments, docs/bootstrap.md) against the numpy restatement
(tests/bootstrap_reference.py) on a 160 x 160 synthetic_scarp with noise, h = 20, w = 1.

Integers - n_blocks, n_profiles, n_failed, every replicate's index, the histogram, lo_index and hi_index - match the
restatement exactly: the draws are integer arithmetic, and a replicate's age is an argmax without a subtraction.  The one
exception is a replicate whose two largest Q_i the restatement finds within 1e-12 relative: such replicates may be at most
0.1 % of a case (bootstrap_reference.compare asserts it on the restatement alone; the seeds and the noise of the cases
were chosen on the CPU so that none has one).  Amplitudes agree within 1e-9 relative, the project's tolerance for fits
against lstsq.  The anchors and the independence of segments are byte comparisons."""
import numpy as np
import pytest

import bootstrap_reference as br
import scarplet_amd as sl
from scarplet_amd import _plan, synthetic

pytestmark = pytest.mark.gpu

CASES = REFS = None
NAMES = ["nb 1 4 5 70", "R 1", "R 1000", "one age", "64 ages", "D 3", "a block of 130", "an empty block", "clipped by the edge"]


def cases():
    global CASES
    if CASES is None:
        CASES = {c["name"]: c for c in br.gpu_cases()}
    return CASES


def ref_of(name):
    """The restatement of a case, computed once and left unchanged."""
    global REFS
    REFS = REFS or {}
    if name not in REFS:
        REFS[name] = br.restate(cases()[name])
    return REFS[name]


def grid(z):
    return sl.DEMGrid.from_array(z, 1.0)


def run(case, cells=None, labels=None, angle=None, **kw):
    args = dict(block_length=case["block_length"], replicates=case["R"], seed=case["seed"], ages=case["ages"],
                min_samples=case["min_samples"], min_blocks=case["min_blocks"], max_shift=float(case["D"]) if case["D"] else None)
    args.update(kw)
    return sl.bootstrap_segments(grid(case["z"]), case["cells"] if cells is None else cells,
                                 case["labels"] if labels is None else labels, case["angle"] if angle is None else angle,
                                 float(br.H), float(br.W), **args)


def test_the_case_list_is_the_one_named_here():
    assert list(cases()) == NAMES
    for c in cases().values():
        assert c["z"].shape == (br.N, br.N) and len(c["cells"]) <= 300


@pytest.mark.parametrize("name", NAMES)
def test_against_the_restatement(name):
    case = cases()[name]
    table, hist, index, amp = run(case, return_hist=True, return_replicates=True)
    S, A, R = len(np.unique(case["labels"])), len(case["ages"]), case["R"]
    assert len(table) == S and hist.shape == (S, A) and hist.dtype == np.int32
    assert index.shape == (S, R + 1) and index.dtype == np.int8 and amp.shape == (S, R + 1)
    ref = ref_of(name)
    st = br.compare(ref, table, hist, index, amp)
    print("%s: %s" % (name, st))
    done = table["status"] != 1
    assert np.array_equal(table["kt0"][done], case["ages"][table["kt_index0"][done]])
    assert np.array_equal(table["kt_lo"][done], case["ages"][table["lo_index"][done]])
    assert np.array_equal(table["kt_hi"][done], case["ages"][table["hi_index"][done]])
    assert np.array_equal(index[:, 0], table["kt_index0"]) and np.array_equal(amp[done, 0], table["a0"][done])
    assert (hist.sum(axis=1) == np.where(done, R - table["n_failed"], 0)).all()
    nb = {r["label"]: r["n_blocks"] for r in ref}
    if name in ("nb 1 4 5 70", "R 1", "R 1000", "one age", "64 ages", "D 3"):
        # 1 and 4 blocks against min_blocks = 5: status 1; 5 blocks; 70: more than one wave of blocks
        assert nb == {2: 4, 4: 70, 6: 1, 9: 5} and case["min_blocks"] == 5
        assert table["status"][[0, 2]].tolist() == [1, 1] and (table["status"][[1, 3]] != 1).all()
        assert table["n_blocks"].tolist() == [4, 70, 1, 5]
    if name == "one age":
        assert (table["status"][[1, 3]] == 6).all() and (index[[1, 3]] == 0).all()
    if name == "64 ages":
        assert A == 64
    if name == "R 1":
        assert np.isnan(table["a_sd"]).all() and (table["a_lo"][done] == table["a_hi"][done]).all()
    if name == "a block of 130":
        # a block whose sum crosses two boundaries of the runs of 64
        assert max(int((br.blocks(case["cells"], br.N, 1.0, br.strike_of(case["angle"]), case["block_length"])[g]).size)
                   for g in range(nb[1])) >= 130 and ref[0]["n_profiles"] == 300
    if name == "an empty block":
        T = ref[0]["terms"]
        assert (T[:, :, 0] == 0).all(axis=1).sum() >= 1 and table["n_blocks"][0] == len(T)     # the empty blocks stay
        assert table["n_profiles"][0] < table["n_cells"][0] and done[0]
    if name == "clipped by the edge":
        assert 0 < table["n_profiles"][0] < table["n_cells"][0] and done[0]
    # a second run and the runs without the optional outputs: the same bytes
    t2, h2, i2, a2 = run(case, return_hist=True, return_replicates=True)
    assert t2.tobytes() == table.tobytes() and h2.tobytes() == hist.tobytes() and i2.tobytes() == index.tobytes()
    assert a2.tobytes() == amp.tobytes()
    assert run(case).tobytes() == table.tobytes()
    t3, h3 = run(case, return_hist=True)
    assert t3.tobytes() == table.tobytes() and h3.tobytes() == hist.tobytes()


@pytest.mark.parametrize("name", ["nb 1 4 5 70", "D 3", "a block of 130", "an empty block"])
def test_replicate_0_is_fit_segments(name):
    """Replicate 0 takes every block once: its index is fit_segments' kt_index and its a fit_segments' a to 1e-9, on the
    same cells, with and without max_shift.  (The restatement finds no near-tie at replicate 0 of these cases.)"""
    case = cases()[name]
    assert not any(r["near"][0] for r in ref_of(name))
    table = run(case)
    fit = sl.fit_segments(grid(case["z"]), case["cells"], case["labels"], case["angle"], float(br.H), float(br.W),
                          ages=case["ages"], min_samples=case["min_samples"], max_shift=float(case["D"]) if case["D"] else None)
    assert np.array_equal(fit["label"], table["label"]) and np.array_equal(fit["n_profiles"], table["n_profiles"])
    done = table["status"] != 1
    assert done.any() and (fit["status"][done] != 1).all()
    assert np.array_equal(table["kt_index0"][done], fit["kt_index"][done])
    assert (np.abs(table["a0"][done] - fit["a"][done]) <= 1e-9 * np.abs(fit["a"][done])).all()
    if case["D"]:
        plain = run(case, max_shift=None)
        assert plain.tobytes() != table.tobytes()
        assert run(case, max_shift=0.0).tobytes() == plain.tobytes()       # D = 0 is the unshifted fit


def test_a_segment_does_not_depend_on_the_others():
    """The rows of a segment are the same bytes whether it is passed alone or with others, and change with its label."""
    case = cases()["nb 1 4 5 70"]
    table, hist, index, amp = run(case, return_hist=True, return_replicates=True)
    for s, L in enumerate(table["label"]):
        pick = case["labels"] == L
        t1, h1, i1, a1 = run(case, cells=case["cells"][pick], labels=case["labels"][pick], angle=case["angle"][pick],
                             return_hist=True, return_replicates=True)
        assert t1.tobytes() == table[s:s + 1].tobytes() and h1.tobytes() == hist[s:s + 1].tobytes()
        assert i1.tobytes() == index[s:s + 1].tobytes() and a1.tobytes() == amp[s:s + 1].tobytes()
    pick = case["labels"] == 4
    t4, i4, a4 = run(case, cells=case["cells"][pick], labels=np.full(pick.sum(), 5), angle=case["angle"][pick],
                     return_replicates=True)
    assert t4["label"][0] == 5 and t4["kt_index0"][0] == table["kt_index0"][1] and t4["a0"][0] == table["a0"][1]
    assert a4[0, 1:].tobytes() != amp[1, 1:].tobytes()


def test_the_seed_changes_the_draws_and_nothing_else():
    case = cases()["nb 1 4 5 70"]
    a, ia, aa = run(case, return_replicates=True)
    b, ib, ab = run(case, seed=case["seed"] + 1, return_replicates=True)
    assert b.tobytes() != a.tobytes() and ab[:, 1:].tobytes() != aa[:, 1:].tobytes()
    assert np.array_equal(ib[:, 0], ia[:, 0]) and ab[:, 0].tobytes() == aa[:, 0].tobytes()
    for f in ("label", "n_cells", "n_profiles", "n_blocks", "kt_index0", "a0"):
        assert a[f].tobytes() == b[f].tobytes(), f
    ref = br.bootstrap_segments(case["z"], 1.0, case["cells"], case["labels"], case["angle"], br.H, br.W, case["ages"],
                                case["block_length"], case["R"], 0.95, case["seed"] + 1, 0, case["min_samples"], 1, 5)
    _, hb, ib2, ab2 = run(case, seed=case["seed"] + 1, return_hist=True, return_replicates=True)
    br.compare(ref, b, hb, ib2, ab2)


def test_both_strike_modes_through_the_matcher():
    """A real search, its traces, and the bootstrap of every segment through the Matcher: the bytes of the free function
    with the same orientations, with strike="cell" and with strike="segment"."""
    g = synthetic.synthetic_scarp(768, theta=0.6)
    m = sl.Matcher(g)
    m.search(sl.Scarp, 100., _plan.age_grid()[::5], _plan.angle_grid())
    res = np.array(m.result_array())
    lo, hi = np.percentile(res[3][res[3] > 0], [60, 90])
    tr = m.extract_traces(lo, hi, 4)
    cells = np.flatnonzero(tr.labels.ravel() > 0)
    assert len(cells) > 50 and len(tr.segments) > 1
    kw = dict(replicates=100, min_blocks=2, seed=11)
    a, ha, ia, aa = m.bootstrap_segments(tr, 60., 5., swath=3., return_hist=True, return_replicates=True, **kw)
    assert np.array_equal(a["label"], tr.segments["label"]) and np.array_equal(a["n_cells"], tr.segments["n_cells"])
    b, hb, ib, ab = sl.bootstrap_segments(g, cells, tr.labels, res[2], 60., 3., block_length=5., return_hist=True,
                                          return_replicates=True, **kw)
    assert a.tobytes() == b.tobytes() and ha.tobytes() == hb.tobytes() and ia.tobytes() == ib.tobytes()
    assert aa.tobytes() == ab.tobytes()
    assert (a["status"] != 1).sum() >= 1
    d = m.bootstrap_segments(tr, 60., 5., swath=3., strike="segment", **kw)
    e = sl.bootstrap_segments(g, cells, tr.labels, tr.segments["strike"][tr.labels.ravel()[cells] - 1], 60., 3.,
                              block_length=5., **kw)
    assert d.tobytes() == e.tobytes() and np.array_equal(d["label"], tr.segments["label"])
    assert d.tobytes() != a.tobytes()
    # replicate 0 through the Matcher is the Matcher's joint fit
    fit = m.fit_segments(tr, 60., 3.)
    done = a["status"] != 1
    assert (np.abs(a["a0"][done] - fit["a"][done]) <= 1e-9 * np.abs(fit["a"][done])).all()
