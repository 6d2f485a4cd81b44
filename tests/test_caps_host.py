"""The cases of tests/caps_cases.py are fair: checked on the CPU, on the restatements alone.

tests/test_gpu_caps.py runs every per-cell call at the top of its accepted range with at most 8 cells a case and the
tolerances of the existing device tests.  Those tolerances stand on conditions that the existing case lists meet by
construction and these cases must meet too: every fitted cell's design matrix under COND_MAX; no decision of the
restatement - the best candidate per age, the best age, both ends of the interval - closer than 1e-6 relative, because with
fewer than 100 cells TIE_SHARE allows no tie at all; sizes that ARE the caps of include/scarplet_hip.h, so that a cap that
moves fails here; the LDS the comments of the kernels say fits; and restatements that take under 30 s."""
import numpy as np
import pytest

import caps_cases as cc
import channel_reference as cr
import profile_reference as pr
import ramp_reference as rr
import robust_reference as ro
import shift_reference as sh
from scarplet_amd import _lib

LIMIT = 30.0                                                               # seconds a case's restatement may take here
LDS = 160 * 1024                                                           # bytes of LDS of a CU


def clear(m):
    """Every margin of ``m`` (a dict or a tuple) above cc.MARGIN."""
    return all(v > cc.MARGIN for v in (m.values() if isinstance(m, dict) else m))


def quick(*keys):
    return sum(cc.SECONDS[k] for k in keys) < LIMIT


# ---- the sizes are the caps -------------------------------------------------------------------------------------------------
def test_the_sizes_of_the_cases_are_the_caps_of_the_header():
    H = cc.header_caps()
    assert H["SC_PROFILE_MAX_SHIFT"] == _lib.PROFILE_MAX_SHIFT and H["SC_PROFILE_MAX_WIDTH"] == _lib.PROFILE_MAX_WIDTH
    assert H["SC_CHANNEL_MAX_FREQS"] == _lib.CHANNEL_MAX_FREQS and H["SC_ROBUST_MAX_ITER"] == _lib.ROBUST_MAX_ITER
    assert H["SC_BOOT_MAX_REPLICATES"] == _lib.BOOT_MAX_REPLICATES
    h, D, q0, q1, _ = cc.LATERAL_ALL
    assert (h, D, q1 - q0 + 1, q1) == (H["SC_PROFILE_MAX_HALF"], H["SC_LATERAL_MAX_LAG"], H["SC_LATERAL_MAX_BAND"],
                                       H["SC_LATERAL_MAX_FAR"])
    one = cc.LATERAL_ONE
    assert one[0][0] == H["SC_PROFILE_MAX_HALF"] and one[0][1] == 0 and one[1][1] == H["SC_LATERAL_MAX_LAG"]
    assert (one[2][3] - one[2][2] + 1, one[2][3]) == (H["SC_LATERAL_MAX_BAND"], H["SC_LATERAL_MAX_FAR"])
    assert (2 * one[3][1] + 1, 2 * one[4][1] + 1) == (255, 257)            # either side of four rounds of 64 ranks
    c = cc.shift_case()
    assert c["D"] == H["SC_PROFILE_MAX_SHIFT"] and len(c["ages"]) == H["SC_PROFILE_MAX_AGES"] and len(c["cells"]) == 8
    assert c["D"] <= c["h"] - c["min_samples"] and c["D"] == 2 ** 6      # +-64: the first value in a signed char's top bits
    for L in (40, 64):
        c = cc.ramp_case(L)
        assert c["M"] == H["SC_PROFILE_MAX_WIDTH"] and len(c["ages"]) == H["SC_PROFILE_MAX_AGES"] and len(c["cells"]) == 6
    ch = cc.channel_cases()
    assert ch["D64"]["D"] == H["SC_PROFILE_MAX_SHIFT"] and len(ch["D64"]["frequencies"]) == H["SC_CHANNEL_MAX_FREQS"]
    assert ch["h1024"]["h"] == H["SC_PROFILE_MAX_HALF"] and len(ch["h1024"]["frequencies"]) == 8 and ch["h1024"]["D"] == 2
    for c in ch.values():
        f = c["frequencies"]
        assert np.all(np.diff(f) > 0) and np.pi * f[-1] * c["de"] <= 6.0 and len(c["cells"]) <= 8
    c = cc.swath_case()
    assert c["w"] == H["SC_PROFILE_MAX_SWATH"] and len(c["ages"]) == 35 and len(c["cells"]) == 8
    assert cc.segment_shift_case()["D"] == H["SC_PROFILE_MAX_SHIFT"] and cc.segment_ramp_case()["M"] == H["SC_PROFILE_MAX_WIDTH"]
    assert cc.bootstrap_case()["R"] == H["SC_BOOT_MAX_REPLICATES"]
    assert cc.ROBUST_T[0] == H["SC_ROBUST_MAX_ITER"]
    for loss in ("huber", "tukey"):
        c = cc.robust_case(loss, 64)
        assert len(c["cells"]) == 6 and len(c["ages"]) == 4 and c["h"] == 100 and c["robust"]["iterations"] == 64


def test_the_lds_the_comments_say_fits_does():
    """sc_lateral.hip: four waves of u, v and the curve at the caps, 163 808 of 163 840 bytes; sc_strike_bootstrap.hip: the
    block terms and the sort padded to 8192 at R = 4096."""
    h, D = cc.LATERAL_ALL[:2]
    assert 8 * 4 * ((2 * h + 1) + (2 * (h + D) + 1) + (2 * D + 1)) == cc.lateral_lds_bytes(h, D) == 163808 <= LDS
    assert cc.lateral_lds_bytes(h + 1, D) > LDS and cc.lateral_lds_bytes(h, D + 1) > LDS   # the caps are where it ends
    assert _lib.STRIKE_BOOT_LDS_TERMS == 16 * 4096
    assert 16 * 4096 + 9 * 8192 == cc.STRIKE_BOOT_LDS_BYTES <= LDS


# ---- 1, 2: lateral -------------------------------------------------------------------------------------------------------------
def test_lateral_at_all_caps_is_decided_clearly_and_in_three_rounds():
    ref = cc.lateral_ref(cc.LATERAL_ALL)
    rows = ref[0]
    gap, near = cc.lateral_margins(ref)
    lag = rows["lag"][:3]
    rank = np.where(lag < 0, -2 * lag - 1, 2 * lag)
    print("lags %s, ranks %s, rounds %s; best against second best %.1e, curve against thr %.1e; %.1f s"
          % (lag.tolist(), rank.tolist(), cc.rounds_of(lag).tolist(), gap, near, cc.SECONDS[("lateral", cc.LATERAL_ALL)]))
    assert rows["status"].tolist()[:3] == [0, 0, 0] and rows["status"][3] == 1 and (rows["n"][:3] == 2049).all()
    assert clear((gap, near))
    assert len(set(cc.rounds_of(lag).tolist())) >= 3 and cc.rounds_of(lag).min() >= 1
    # a winner past the first round in the upper half of the lanes: a lane taken from fewer than six bits of the rank is wrong
    assert ((rank >= 64) & (rank % 64 >= 32)).any()
    assert quick(("lateral", cc.LATERAL_ALL))


@pytest.mark.parametrize("p", cc.LATERAL_ONE, ids=lambda p: "h%d-D%d-q%d_%d" % p[:4])
def test_lateral_one_cap_at_a_time_is_decided_clearly(p):
    ref = cc.lateral_ref(p)
    rows = ref[0]
    gap, near = cc.lateral_margins(ref)
    print("%r: n %s, lags %s; margins %.1e %.1e" % (p, rows["n"].tolist(), rows["lag"].tolist(), gap, near))
    assert (rows["status"][:3] & 1 == 0).all()                             # (the corner is fitted where half a profile is enough)
    assert clear((gap, near))                                            # (D = 0: one lag, the gap is inf)
    assert quick(("lateral", p))


# ---- 3: the centre shift ----------------------------------------------------------------------------------------------------------
def test_shift_64_is_conditioned_clear_and_spread():
    ref = cc.shift_ref()
    m = cc.shift_margins(ref)
    d = [r["shift_index"] for r in ref]
    print("shifts %s, status %s, cond %.1f, margins %s, %.1f s" % (d, [r["status"] for r in ref], max(r["cond"] for r in ref), m,
                                                                  cc.SECONDS["shift ref"]))
    assert all(r["status"] != 1 and r["n"] == 321 for r in ref) and max(r["cond"] for r in ref) <= sh.COND_MAX
    assert clear(m) and cc.spread_of(d, 64) and ref[-1]["status"] & 8
    # the winners of the best age sit past rank 64 of the (candidate, age) order, and in many different rounds of lanes
    assert sum(abs(v) > 8 for v in d) >= 6
    assert quick("shift ref")


# ---- 4: the ramp ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [40, 64])
@pytest.mark.parametrize("mode", [rr.FREE, rr.SLOPE], ids=["free", "slope"])
def test_ramp_64_is_conditioned_and_clear(L, mode):
    c = cc.ramp_case(L)
    ref = cc.ramp_ref(L, mode)
    m = cc.ramp_margins(ref, mode, c["slope"])
    print("L %d mode %d: widths %s, status %s, cond %.1f, margins %s" % (L, mode, [r["width_index"] for r in ref],
                                                                        [r["status"] for r in ref], max(r["cond"] for r in ref), m))
    assert max(r["cond"] for r in ref) <= rr.COND_MAX and clear(m)
    assert all(r["width_index"] == L for r in ref) and all(bool(r["status"] & 8) == (L == 64) for r in ref)
    # the float64 restatement is no worse than RTOL / 100 from its longdouble twin here, as ramp_reference.NA asks
    worst = 0.0
    for a, b in zip(cc.ramp_ref(L, rr.FREE), cc.kept(("ramp longdouble", L), lambda: rr.restate(c, rr.FREE, longdouble=True))):
        g = np.asarray(b["grid"], dtype=np.float64)
        worst = max(worst, float(np.max(np.abs(a["grid"] - g) / g)))
    assert worst <= rr.RTOL / 100, worst
    assert cc.SECONDS.get(("ramp ref", L, rr.FREE), 0.0) + cc.SECONDS[("ramp longdouble", L)] < LIMIT


# ---- 5: channels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["D64", "h1024"])
def test_channels_are_conditioned_clear_and_spread(which):
    c = cc.channel_cases()[which]
    ref = cc.kept(("channel ref", which), lambda: cr.restate(c))
    m = cc.channel_margins(ref)
    d = [r["shift_index"] for r in ref]
    print("%s: shifts %s, f_index %s, cond %.1f, margins %s, %.1f s" % (which, d, [r["f_index"] for r in ref],
                                                                       max(r["cond"] for r in ref), m, cc.SECONDS[("channel ref", which)]))
    assert all(r["status"] & 1 == 0 and r["n"] == 2 * c["h"] + 1 for r in ref) and max(r["cond"] for r in ref) <= cr.COND_MAX
    assert not any(np.isnan(r["curve"]).any() for r in ref) and clear(m)
    if which == "D64":
        assert cc.spread_of(d, 64) and ref[-1]["status"] & 8
    assert quick(("channel ref", which))


# ---- 6: the swath -----------------------------------------------------------------------------------------------------------------
def test_swath_32_leaves_the_grid_meets_nan_cells_and_is_clear():
    c = cc.swath_case()
    ref = cc.swath_ref()
    m = cc.swath_margins(ref)
    print("n %s, kt_index %s, cond %.1f, margins %s" % ([r["n"] for r in ref], [r["kt_index"] for r in ref],
                                                       max(r["cond"] for r in ref), m))
    assert all(r["status"] != 1 for r in ref) and max(r["cond"] for r in ref) <= pr.COND_MAX and clear(m)
    # lines of the swath that leave the grid or meet NaN cells change the mean of a point: against a swath of 5, and
    # against the surface without the hole
    nx = c["z"].shape[1]
    whole = pr.synthetic_z(400, seed=11)
    sa, ca = np.sin(0.2), np.cos(0.2)
    profile = lambda z, cell, w: pr.sample_profile(z, float(cell // nx), float(cell % nx), sa, ca, c["h"], w)
    holed = [not np.array_equal(profile(c["z"], int(cell), 32), profile(whole, int(cell), 32)) for cell in c["cells"]]
    assert sum(holed) >= 2 and not all(holed)
    top = int(c["cells"][0])
    k = np.arange(-32, 33)
    inside = (top // nx + k * ca >= 0).sum()                               # the 65 lines of the point j = 0, six rows from the top
    assert top // nx < 10 and 32 < inside < 65
    assert quick("swath ref")


# ---- 7: segments ------------------------------------------------------------------------------------------------------------------
def test_segments_at_the_caps_are_conditioned_and_clear():
    single = cc.shift_ref()
    ref = cc.kept("segment shift ref", lambda: cc.segment_shift_ref(np.stack([r["shifts"] for r in single])))
    m = cc.segment_margins(ref)
    print("shift: kt_index %s, status %s, cond %.1f, margins %s" % ([r["kt_index"] for r in ref], [r["status"] for r in ref],
                                                                   max(r["cond"] for r in ref), m))
    assert len(ref) == 2 and all(r["n_profiles"] == 4 for r in ref) and max(r["cond"] for r in ref) <= sh.COND_MAX and clear(m)
    assert quick("segment shift ref")
    for mode in (rr.FREE, rr.SLOPE):
        c = cc.segment_ramp_case()
        ref = cc.segment_ramp_ref(40, mode)
        m = cc.segment_ramp_margins(ref, mode, c["slope"])
        print("ramp, mode %d: widths %s, cond %.1f, margins %s" % (mode, [r["width_index"] for r in ref],
                                                                  max(r["cond"] for r in ref), m))
        assert len(ref) == 2 and all(r["n_profiles"] == 3 and r["width_index"] == 40 for r in ref)
        assert max(r["cond"] for r in ref) <= rr.COND_MAX and clear(m)
    assert quick(("segment ramp ref", 40, rr.FREE))


# ---- 8: the segment bootstrap -----------------------------------------------------------------------------------------------------
def test_bootstrap_4096_has_no_near_tie():
    ref = cc.bootstrap_ref()
    done = [r for r in ref if r["status"] != 1]
    print("%d segments booted, %d near-ties, %.1f s" % (len(done), sum(int(r["near"].sum()) for r in done), cc.SECONDS["bootstrap ref"]))
    assert len(done) == 2 and all(r["replicates"] == 4096 and len(r["index"]) == 4097 for r in done)
    assert sum(int(r["near"].sum()) for r in done) == 0
    assert quick("bootstrap ref")


# ---- 9: robust --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["huber", "tukey"])
def test_two_restatements_agree_after_the_reweightings(loss):
    """Whether two correct implementations agree within 1e-9 after 64 reweightings is decided here, by the float64 and
    the longdouble restatement, not by the device: the device case runs at the T this finds (profiles/caps.txt)."""
    T, d = cc.robust_iterations(loss, ro.RTOL / 10)
    print("%s: the restatements agree within %.1e at T = %s" % (loss, d, T))
    assert T is not None, d
    ref = cc.robust_refs(loss, T)[0]
    m = cc.robust_margins(ref)
    print("kt_index %s, n_down %s, cond %.1f, margins %s" % ([r["kt_index"] for r in ref], [r["n_down"] for r in ref],
                                                            max(r["cond"] for r in ref), m))
    assert all(r["status"] & 49 == 0 for r in ref) and max(r["cond"] for r in ref) <= ro.COND_MAX and clear(m)
    assert any(r["n_down"] > 0 for r in ref)
    assert quick(("robust ref", loss, T))
