"""Every per-cell call at the top of its accepted range on the MI355X (include/scarplet_hip.h: half-length 1024, swath 32,
64 ages or frequencies, centre shift 64, ramp half-width 64, lateral lag 255 with 64 lines out to 1024 cells, 64 robust
iterations, 4096 replicates) against the existing numpy restatements.

The cases are tests/caps_cases.py's, at most 8 cells or stations each; tests/test_caps_host.py shows on the CPU that they
stand on the ground of the tolerances used here - which are the restatements' own, through their own compare functions:
1e-9 relative, integers exact, COND_MAX and TIE_SHARE as each module defines them (with so few cells: no tie).  What the
caps reach and smaller sizes do not: 163 808 bytes of LDS and eight rounds of lag ranks in k_lt_fit, 129 rounds of the
(candidate, age) pairs in sh_search / rp_search and winners of rank > 64 in them, +-64 in the signed char planes, the far
rows of the erf and F tables, 65 lines a point in pf_point and a sort padded to 8192 in the segment bootstrap."""
import time

import numpy as np
import pytest

import bootstrap_reference as br
import caps_cases as cc
import channel_reference as cr
import profile_reference as pr
import ramp_reference as rr
import robust_reference as ro
import segment_ramp_reference as sx
import shift_reference as sh
import test_gpu_lateral as tl
import scarplet_amd as sl
from scarplet_amd import core

pytestmark = pytest.mark.gpu


def grid(z, de=1.0):
    return sl.DEMGrid.from_array(z, float(de))


def timed(fn):
    """(what fn() returns, the seconds it took): printed with each case's figures."""
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def same_bytes(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


# ---- 1, 2: sl.lateral_offsets ------------------------------------------------------------------------------------------------
def lateral(p, cells=None, ang=None, **kw):
    h, D, q0, q1, ms = p
    c0, a0 = cc.lateral_stations()
    return sl.lateral_offsets(grid(cc.lateral_dem()), c0 if cells is None else cells, a0 if ang is None else ang, float(h),
                              float(q0), float(q1), float(D), min_samples=ms, **kw)


def test_lateral_at_all_caps():
    """h 1024, lag 255, 64 lines out to 1024 cells: four waves of 5119 doubles, 163 808 of the CU's 163 840 bytes of LDS;
    eight rounds of 64 lag ranks, the winners in three different rounds past the first."""
    p = cc.LATERAL_ALL
    ref = cc.lateral_ref(p)
    tl.assert_no_near_ties(*ref)
    (table, curve), sec = timed(lambda: lateral(p, return_curve=True))
    print("lateral %r: lags %s, n %s, status %s, %.3f s" % (p, table["lag"].tolist(), table["n"].tolist(),
                                                           table["status"].tolist(), sec))
    worst = tl.compare(ref, table, curve)
    print("lateral %r: worst relative difference %.2e" % (p, worst))
    assert curve.shape == (4, 2 * p[1] + 1) and (table["status"][:3] & 1 == 0).all() and table["status"][3] == 1
    rounds = cc.rounds_of(table["lag"][:3])
    assert len(set(rounds.tolist())) >= 3, rounds
    # the same stations in another order, and without the curves: the same bytes
    cells, ang = cc.lateral_stations()
    perm = np.array([2, 3, 0, 1])
    t2, c2 = lateral(p, cells[perm], ang[perm], return_curve=True)
    assert t2.tobytes() == table[perm].tobytes() and c2.tobytes() == curve[perm].tobytes()
    assert lateral(p).tobytes() == table.tobytes()


@pytest.mark.parametrize("p", cc.LATERAL_ONE, ids=lambda p: "h%d-D%d-q%d_%d" % p[:4])
def test_lateral_one_cap_at_a_time(p):
    """Which dimension fails, if the case above does; 255 and 257 lags are either side of a round of ranks."""
    ref = cc.lateral_ref(p)
    tl.assert_no_near_ties(*ref)
    (table, curve), sec = timed(lambda: lateral(p, return_curve=True))
    worst = tl.compare(ref, table, curve)
    print("lateral %r: lags %s, n %s, worst relative difference %.2e, %.3f s" % (p, table["lag"].tolist(), table["n"].tolist(),
                                                                                worst, sec))
    assert (table["status"][:3] & 1 == 0).all()
    assert lateral(p).tobytes() == table.tobytes()


# ---- 3: the centre shift at D = 64 -------------------------------------------------------------------------------------------
def run_shift(case, **kw):
    h, w, de = case["h"], case["w"], case["de"]
    return sl.fit_profiles(grid(case["z"], de), case["cells"], case["angle"], h * de, w * de, ages=case["ages"],
                           delta=case["delta"], min_samples=case["min_samples"], max_shift=case["D"] * de, **kw)


def test_shift_64():
    """129 candidates x 64 ages: 129 rounds of sh_search, winners at ranks up to 128, +-64 in the shift plane, the far rows of
    the erf table."""
    case = cc.shift_case()
    (table, curve, shifts), sec = timed(lambda: run_shift(case, return_curve=True, return_shift=True))
    print("shift 64: winners %s, status %s, %.3f s" % (table["shift_index"].tolist(), table["status"].tolist(), sec))
    assert shifts.dtype == np.int8 and shifts.shape == (8, 64)
    st = sh.compare_rows(cc.shift_ref(), table, curve, shifts, case["h"], case["de"], case["D"], case["delta"])
    print("shift 64: %s" % st)
    assert st["fitted"] == 8 and st["ties"] == 0
    d = table["shift_index"]
    assert (d >= 48).any() and (d <= -48).any() and (np.abs(d) == 64).any() and (table["status"][np.abs(d) == 64] & 8 == 8).all()
    assert shifts.min() == -64 and shifts.max() >= 63
    same_bytes(run_shift(case, return_curve=True, return_shift=True), (table, curve, shifts))
    assert run_shift(case).tobytes() == table.tobytes()


# ---- 4: the ramp at M = 64 ---------------------------------------------------------------------------------------------------
def run_ramp(case, mode, **kw):
    h, w, de = case["h"], case["w"], case["de"]
    if mode == rr.SLOPE:
        kw["initial_slope"] = case["slope"]
    return sl.fit_profiles(grid(case["z"], de), case["cells"], case["angle"], h * de, w * de, ages=case["ages"],
                           delta=case["delta"], min_samples=case["min_samples"], max_width=case["M"] * de, **kw)


@pytest.mark.parametrize("L", [40, 64])
@pytest.mark.parametrize("mode", [rr.FREE, rr.SLOPE], ids=["free", "slope"])
def test_ramp_64(L, mode):
    """65 half-widths x 64 ages: rows (M +- m) A + i of the table of F out to m = 64; a planted half-width of 40 cells, and
    one of 64, which wins at the end of the range and sets bit 8."""
    case = cc.ramp_case(L)
    (table, curve, widths), sec = timed(lambda: run_ramp(case, mode, return_curve=True, return_width=True))
    print("ramp L %d mode %d: widths %s, status %s, %.3f s" % (L, mode, table["width_index"].tolist(), table["status"].tolist(), sec))
    assert widths.dtype == np.int8 and widths.shape == (6, 64)
    st = rr.compare_rows(cc.ramp_ref(L, mode), table, curve, widths, case["h"], case["de"], case["M"], mode, case["slope"],
                         case["delta"])
    print("ramp L %d mode %d: %s" % (L, mode, st))
    assert st["fitted"] == 6 and st["ties"] == 0
    assert (table["width_index"] == L).all() and ((table["status"] & 8 == 8) == (L == 64)).all()
    same_bytes(run_ramp(case, mode, return_curve=True, return_width=True), (table, curve, widths))
    assert run_ramp(case, mode).tobytes() == table.tobytes()


# ---- 5: sl.fit_channels ------------------------------------------------------------------------------------------------------
def run_channels(case, **kw):
    h, w, de = case["h"], case["w"], case["de"]
    return sl.fit_channels(grid(case["z"], de), case["cells"], case["angle"], h * de, case["frequencies"], swath=w * de,
                           max_shift=case["D"] * de, delta=case["delta"], min_samples=case["min_samples"], **kw)


@pytest.mark.parametrize("which", ["D64", "h1024"])
def test_channels(which):
    case = cc.channel_cases()[which]
    ref = cc.kept(("channel ref", which), lambda: cr.restate(case))
    (table, curve, shifts), sec = timed(lambda: run_channels(case, return_curve=True, return_shift=True))
    print("channels %s: shifts %s, f_index %s, status %s, %.3f s" % (which, table["shift_index"].tolist(), table["f_index"].tolist(),
                                                                    table["status"].tolist(), sec))
    st = cr.compare_rows(ref, table, curve, shifts, case["h"], case["de"], case["D"], case["delta"])
    print("channels %s: %s" % (which, st))
    assert st["fitted"] == len(case["cells"]) and st["ties"] == 0 and st["dead"] == 0
    if which == "D64":
        d = table["shift_index"]
        assert (d >= 48).any() and (d <= -48).any() and (np.abs(d) == 64).any()
        assert (table["status"][np.abs(d) == 64] & 8 == 8).all() and shifts.min() == -64
    # every profile is complete: the terms table serves them all, and sweeping for the terms instead changes no byte
    assert (table["n"] == 2 * case["h"] + 1).all()
    ctx = core._context(0)
    ctx.set_option("channel_terms", 0)
    try:
        slow = run_channels(case, return_curve=True, return_shift=True)
    finally:
        ctx.set_option("channel_terms", 1)
    same_bytes(slow, (table, curve, shifts))
    assert run_channels(case).tobytes() == table.tobytes()


# ---- 6: a swath of 32 --------------------------------------------------------------------------------------------------------
def test_swath_32():
    """65 lines a point in pf_point: in the interior, six rows from the top - part of the swath outside - and next to NaN cells."""
    case = cc.swath_case()
    h, w, de = case["h"], case["w"], case["de"]
    run = lambda **kw: sl.fit_profiles(grid(case["z"], de), case["cells"], case["angle"], h * de, w * de, ages=case["ages"],
                                       delta=case["delta"], min_samples=case["min_samples"], **kw)
    (table, curve), sec = timed(lambda: run(return_curve=True))
    got = [dict({f: table[f][k] for f in table.dtype.names}, curve=curve[k]) for k in range(len(table))]
    st = pr.compare_rows(cc.swath_ref(), got, h, de, case["delta"])
    print("swath 32: kt_index %s, %s, %.3f s" % (table["kt_index"].tolist(), st, sec))
    assert st["fitted"] == 8 and st["ties"] == 0
    assert run().tobytes() == table.tobytes()


# ---- 7: the segment fits at the caps -----------------------------------------------------------------------------------------
def run_segments(case, labels=None, mode=rr.FREE, **kw):
    h, w, de = case["h"], case["w"], case["de"]
    if "D" in case:
        kw["max_shift"] = case["D"] * de
    else:
        kw["max_width"] = case["M"] * de
        kw["initial_slope"] = case["slope"] if mode == rr.SLOPE else None
    return sl.fit_segments(grid(case["z"], de), case["cells"], case["labels"] if labels is None else labels, case["angle"], h * de,
                           w * de, ages=case["ages"], delta=case["delta"], min_samples=case["min_samples"],
                           min_profiles=case["min_profiles"], **kw)


def test_segments_shift_64():
    case = cc.segment_shift_case()
    (table, cells, curve, shifts), sec = timed(lambda: run_segments(case, return_cells=True, return_curve=True, return_shift=True))
    # stage one: every d_ci against the single-profile restatement; stage two: the joint fit with those shifts
    for k, r in enumerate(cc.shift_ref()):
        assert sh.check_shifts(r, shifts[k]) == 0
    ref = cc.segment_shift_ref(shifts)
    assert np.array_equal(cells["cell"], case["cells"]) and np.array_equal(cells["label"], case["labels"])
    st = sh.compare_segments(ref, table, cells, curve, case["h"], case["de"], case["D"], case["delta"])
    print("segments, shift 64: shifts %s, kt_index %s, status %s, %s, %.3f s"
          % (cells["shift_index"].tolist(), table["kt_index"].tolist(), table["status"].tolist(), st, sec))
    assert st["fitted"] == 2 and st["ties"] == 0 and shifts.min() == -64 and (np.abs(cells["shift_index"]) >= 48).any()
    # one-cell segments return the bytes of the single fit
    lab = np.random.default_rng(3).permutation(8) + 1
    seg, ct, cv, sp = run_segments(case, labels=lab, return_cells=True, return_curve=True, return_shift=True)
    one, ocv, osp = run_shift(case, return_curve=True, return_shift=True)
    assert sp.tobytes() == osp.tobytes() == shifts.tobytes()
    for f in ("b", "c0", "sse", "shift_index", "shift", "cell", "n"):
        assert ct[f].tobytes() == one[f].tobytes(), f
    one, ocv = one[np.argsort(lab)], ocv[np.argsort(lab)]
    for f in ("kt_index", "lo_index", "hi_index", "status", "a", "sse", "rmse", "kt", "kt_lo", "kt_hi", "height"):
        assert seg[f].tobytes() == one[f].tobytes(), f
    assert cv.tobytes() == ocv.tobytes() and np.array_equal(seg["dof"], one["n"] - 4) and (seg["n_cells"] == 1).all()
    assert (one["status"] != 1).all()


@pytest.mark.parametrize("mode", [rr.FREE, rr.SLOPE], ids=["free", "slope"])
def test_segments_ramp_64(mode):
    case = cc.segment_ramp_case()
    (table, cells, curve, widths), sec = timed(lambda: run_segments(case, mode=mode, return_cells=True, return_curve=True,
                                                                   return_width=True))
    assert np.array_equal(cells["cell"], case["cells"]) and np.array_equal(cells["label"], case["labels"])
    st = sx.compare_segments(cc.segment_ramp_ref(40, mode), table, cells, curve, widths, case["h"], case["de"], case["M"], mode,
                             case["slope"], case["delta"])
    print("segments, ramp 64, mode %d: widths %s, kt_index %s, %s, %.3f s" % (mode, table["width_index"].tolist(),
                                                                             table["kt_index"].tolist(), st, sec))
    assert st["fitted"] == 2 and st["ties"] == 0 and (table["width_index"] == 40).all()
    # one-cell segments return the bytes of the single fit
    lab = np.random.default_rng(3).permutation(6) + 1
    seg, ct, cv, wp = run_segments(case, labels=lab, mode=mode, return_cells=True, return_curve=True, return_width=True)
    one, ocv, owp = run_ramp(case, mode, return_curve=True, return_width=True)
    for f in ("b", "c0", "sse", "cell", "n"):
        assert ct[f].tobytes() == one[f].tobytes(), f
    order = np.argsort(lab)
    one, ocv, owp = one[order], ocv[order], owp[order]
    for f in ("kt_index", "lo_index", "hi_index", "status", "a", "sse", "rmse", "kt", "kt_lo", "kt_hi", "height", "width_index",
              "width", "initial_slope"):
        assert seg[f].tobytes() == one[f].tobytes(), f
    assert cv.tobytes() == ocv.tobytes() and wp.tobytes() == owp.tobytes() and (one["status"] != 1).all()
    assert np.array_equal(seg["dof"], one["n"] - 3 - (1 if mode == rr.FREE else 0)) and (seg["n_cells"] == 1).all()


# ---- 8: sl.bootstrap_segments at R = 4096 ------------------------------------------------------------------------------------
def test_bootstrap_segments_4096():
    """The sort of the replicates' amplitudes padded to 8192."""
    case = cc.bootstrap_case()
    run = lambda **kw: sl.bootstrap_segments(grid(case["z"]), case["cells"], case["labels"], case["angle"], float(br.H),
                                             float(br.W), block_length=case["block_length"], replicates=case["R"],
                                             seed=case["seed"], ages=case["ages"], min_samples=case["min_samples"],
                                             min_blocks=case["min_blocks"], max_shift=None, **kw)
    (table, hist, index, amp), sec = timed(lambda: run(return_hist=True, return_replicates=True))
    assert index.shape == (4, 4097) and amp.shape == (4, 4097) and hist.shape == (4, len(case["ages"]))
    st = br.compare(cc.bootstrap_ref(), table, hist, index, amp)
    print("bootstrap_segments R 4096: %s, lo %s hi %s, %.3f s" % (st, table["lo_index"].tolist(), table["hi_index"].tolist(), sec))
    assert st["booted"] == 2 and st["flipped"] == 0 and st["near"] == 0 and table["n_blocks"].tolist() == [4, 70, 1, 5]
    assert run().tobytes() == table.tobytes()


# ---- 9: robust=, 64 iterations -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["huber", "tukey"])
def test_robust_at_the_most_iterations_two_restatements_agree_on(loss):
    """T is the largest of 64, 32, 16 at which the float64 and the longdouble restatement agree within RTOL / 10 on these
    inputs (tests/test_caps_host.py; profiles/caps.txt: 64).  The tolerance for the device is robust_reference's."""
    T, d = cc.robust_iterations(loss, ro.RTOL / 10)
    assert T is not None, d
    case = cc.robust_case(loss, T)
    run = lambda: sl.fit_profiles(grid(case["z"], case["de"]), case["cells"], case["angle"], case["h"] * case["de"],
                                  case["w"] * case["de"], return_curve=True, ages=case["ages"], delta=case["delta"],
                                  min_samples=case["min_samples"], weights=case["weights"], **case["robust"])
    (table, curve), sec = timed(run)
    got = [dict({f: table[f][k] for f in table.dtype.names}, curve=curve[k]) for k in range(len(table))]
    st = ro.compare_rows(case, cc.robust_refs(loss, T)[0], got)
    print("robust %s, T %d (restatements within %.1e): kt_index %s, n_down %s, %s, %.3f s"
          % (loss, T, d, table["kt_index"].tolist(), table["n_down"].tolist(), st, sec))
    assert st["fitted"] == 6 and st["ties"] == 0
    t2, c2 = run()
    assert t2.tobytes() == table.tobytes() and c2.tobytes() == curve.tobytes()
