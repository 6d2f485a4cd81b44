"""numpy restatement of sc_channel_strike / sl.fit_channels_along_strike (docs/channels.md, "Width along a reach"),
algebraically independent of the device's route.  The hand-over is ``strike.windows_of`` on the cells grouped by label - the
strike of a reach is ``bootstrap_reference.strike_of``, the axial mean of its cells' angles in input order - and every
window's row is ``channel_segment_reference.fit_reach`` on the stage-one records of the window's cells in hand-over order:
ONE float64 ``lstsq`` on the full, column-scaled design matrix per window and frequency, never the per-profile term sums of
the device and never ``SSpp - Q``.  ``shift_sum`` comes from the records: the sum of the usable profiles' ``d_ci`` at the
window's best frequency."""
import numpy as np

import bootstrap_reference as br
import channel_bootstrap_reference as cb
import channel_reference as cr
import channel_segment_reference as csr
import strike_reference as stk
from scarplet_amd import strike

RTOL, COND_MAX, TIE_SHARE = csr.RTOL, csr.COND_MAX, csr.TIE_SHARE
SPP_MAX = stk.SPP_MAX      # a condition on the inputs, segment mode: SSpp / sse_min of every compared window
MODES = csr.MODES
ROW_INTS = ("label", "station", "n_cells", "n_profiles", "n", "dof")
ROW_FLOATS = csr.ROW_FLOATS
DERIVED = csr.DERIVED


# ---- the hand-over -------------------------------------------------------------------------------------------------------------
def handover(case):
    """(labels, order, seg_win_start, win_lo, win_hi, centre): the ascending labels > 0, the input positions of the kept cells
    in hand-over order, and ``strike.windows_of``'s windows as ranges of that order."""
    lab, where = csr.group(case["labels"])
    nx = case["z"].shape[1]
    pos = np.concatenate(where) if len(where) else np.zeros(0, dtype=np.int64)
    seg_start = np.concatenate([[0], np.cumsum([len(p) for p in where])]).astype(np.int64)
    strikes = [br.strike_of(case["angle"][p]) for p in where]
    by, _, sws, lo, hi, centre = strike.windows_of(case["cells"][pos], nx, case["de"], strikes, seg_start, case["window"],
                                                   case["step"])
    return lab, pos[by], sws, lo, hi, centre


# ---- stage one and Spp, per cell, shared by the cases that cut different windows from the same cells ----------------------------
_STAGE, _ROWS = {}, {}


def stage_of(case):
    """``channel_segment_reference.stage_cell`` of every kept cell, plus 'spp' of a usable one (strike_reference.spp_of)."""
    key = case.get("stage", case["name"])
    if key not in _STAGE:
        sa, ca = np.sin(case["angle"]), np.cos(case["angle"])
        out = []
        for k in range(len(case["cells"])):
            if case["labels"][k] <= 0:
                out.append(None)
                continue
            c = csr.stage_cell(case["z"], case["de"], case["cells"][k], sa[k], ca[k], case["h"], case["w"], case["D"],
                               case["frequencies"], case["min_samples"])
            if c["usable"]:
                c["spp"] = stk.spp_of(case["z"], case["cells"][k], sa[k], ca[k], case["h"], case["w"], case["de"],
                                      case["min_samples"])
            out.append(c)
        _STAGE[key] = out
    return _STAGE[key]


def restate(case, mode):
    """The restatement's rows of a case, one per (label, station) in that order: fit_reach's fields plus 'label', 'station',
    't', 'row', 'col', 'where' (the input positions of the window's cells in hand-over order), 'shift_sum' and 'spp'."""
    key = (case["name"], mode)
    if key in _ROWS:
        return _ROWS[key]
    st = stage_of(case)
    nx = case["z"].shape[1]
    lab, order, sws, lo, hi, centre = handover(case)
    rows = []
    for s, L in enumerate(lab):
        for g in range(int(sws[s]), int(sws[s + 1])):
            wp = order[lo[g]:hi[g]]
            recs = [st[k] for k in wp]
            row = csr.fit_reach(recs, case["de"], case["D"], case["frequencies"], mode, case["delta"], case["min_profiles"])
            us = [c for c in recs if c["usable"]]
            fitted = row["status"] & 1 == 0
            row.update(label=int(L), station=g - int(sws[s]), t=float(centre[g]), where=wp,
                       row=float(np.mean(case["cells"][wp] // nx)) if len(wp) else np.nan,
                       col=float(np.mean(case["cells"][wp] % nx)) if len(wp) else np.nan,
                       shift_sum=sum(int(c["shifts"][row["f_index"]]) for c in us) if fitted else 0,
                       spp=float(sum(c["spp"] for c in us)))
            rows.append(row)
    _ROWS[key] = rows
    return rows


# ---- comparing the device's table with the restatement ---------------------------------------------------------------------------
def compare(ref, mode, table, curve, de):
    """The device's table and (NW, F) curves against ``ref`` (restate's rows), by channel_segment_reference.compare's rules:
    integers, statuses and dead-frequency masks are equal except in a window whose margin is <= RTOL, which counts as a tie;
    floats and curves are within RTOL, ``a`` scaled by the window's largest peak-to-peak range.  Asserts - the conditions on
    the inputs too -; returns the figures."""
    out = {"windows": len(ref), "fitted": 0, "ties": 0, "sse": 0.0, "a": 0.0, "cond": 0.0, "spp": 0.0, "dead": 0, "margin": np.inf}
    assert len(table) == len(ref) and curve.shape[0] == len(ref)
    for s, (r, g) in enumerate(zip(ref, table)):
        key = (r["label"], r["station"])
        for f in ROW_INTS:
            assert int(g[f]) == r[f], (key, f, g[f], r[f])
        assert abs(float(g["t"]) - r["t"]) <= 1e-12 * max(1.0, abs(r["t"])), (key, g["t"], r["t"])
        for f in ("row", "col"):
            assert (np.isnan(g[f]) and np.isnan(r[f])) or abs(float(g[f]) - r[f]) <= 1e-12 * max(1.0, abs(r[f])), (key, f)
        tie = r["margin"] <= RTOL
        out["margin"] = min(out["margin"], r["margin"])
        out["ties"] += bool(tie)
        if r["status"] & 1:
            if not tie:
                assert int(g["status"]) == r["status"], (key, g["status"], r["status"])
                assert int(g["f_index"]) == -1 and int(g["lo_index"]) == -1 and int(g["hi_index"]) == -1, key
                assert all(np.isnan(g[f]) for f in ROW_FLOATS + DERIVED + ("shift_mean",)), key
                assert np.isnan(curve[s]).all(), key
            continue
        out["fitted"] += 1
        cv, dof = r["curve"], r["dof"]
        assert r["cond"] <= COND_MAX, ("the inputs leave the tolerance's ground", key, r["cond"])
        out["cond"] = max(out["cond"], r["cond"])
        if mode == "segment":
            assert r["spp"] <= SPP_MAX * np.nanmin(cv), ("the inputs leave the tolerance's ground", key, r["spp"] / np.nanmin(cv))
            out["spp"] = max(out["spp"], r["spp"] / np.nanmin(cv))
        if tie:
            continue
        dead = np.isnan(cv)
        out["dead"] += int(dead.sum())
        assert np.array_equal(np.isnan(curve[s]), dead), (key, "dead frequencies")
        gi = int(g["f_index"])
        assert (gi, int(g["lo_index"]), int(g["hi_index"]), int(g["status"])) == \
            (r["f_index"], r["lo_index"], r["hi_index"], r["status"]), (key, g, r["f_index"], r["lo_index"], r["hi_index"], r["status"])
        assert float(g["f"]) == r["f"] and float(g["f_lo"]) == r["f_lo"] and float(g["f_hi"]) == r["f_hi"], key
        ds = max(abs(float(g["sse"]) - cv[gi]) / cv[gi], float(np.max(np.abs(curve[s][~dead] - cv[~dead]) / cv[~dead])))
        da = abs(float(g["a"]) - r["a"]) / r["ptp"]
        assert ds <= RTOL, (key, "sse", ds)
        assert da <= RTOL, (key, "a", da)
        assert float(g["sse"]) == curve[s][gi] and float(g["rmse"]) == float(np.sqrt(g["sse"] / dof)), key
        assert float(g["depth"]) == -float(g["a"]), key
        assert float(g["shift_mean"]) == de * r["shift_sum"] / r["n_profiles"], (key, g["shift_mean"], r["shift_sum"])
        out["sse"], out["a"] = max(out["sse"], ds), max(out["a"], da)
    assert out["ties"] <= TIE_SHARE * max(1, out["windows"]), out
    return out


# ---- the recovery of docs/channels.md, "Width along a reach" ---------------------------------------------------------------------
# channel_bootstrap_reference's widening trough - sigma = 1.5 * 1.12^(14 + span c), c = clip(xrot / 150, -1, 1) - in windows
# of 60 every 30: the planted index of a cell is 27 - (14 + span c)
REC_WINDOW, REC_STEP = 60.0, 30.0
REC_PROFILES = [11, 20, 19, 19, 20, 20, 20, 19, 19, 20, 11]
# ... as the restatement measures it (tests/test_channel_strike_host.py), in both depth modes
REC_INDEX = {3: [16, 15, 15, 14, 14, 13, 12, 12, 11, 11, 10], 0: [13] * 11}


def recovery(span):
    c = cb.widening_case(span)
    return dict(c, name="along strike, " + c["name"], stage="along strike, " + c["stage"], window=REC_WINDOW, step=REC_STEP)


def planted_index(case, span):
    """The planted frequency index 27 - (14 + span c) of every cell of the widening trough."""
    n, theta = cb.WIDE["n"], cb.WIDE["theta"]
    x = np.linspace(-n / 2, n / 2, num=n, dtype=np.float64)
    th = np.pi / 2 - theta
    r, c = case["cells"] // n, case["cells"] % n
    xrot = x[c] * np.cos(th) + x[r] * np.sin(th)
    return 27.0 - (14.0 + span * np.clip(xrot / cb.WIDE["reach"], -1.0, 1.0))


# ---- the inputs of tests/test_gpu_channel_strike.py -------------------------------------------------------------------------------
N = 300
NAMES = ["run %d" % c for c in stk.RUNS] + \
    ["unusable", "unusable min_profiles 3", "F = 1", "F = 64, h = 100, D = 8", "D = 0", "D = h - min_samples", "de = 2",
     "several reaches", "NaN holes", "a hole at the centre at pi f de = 6", "every frequency dead"]
_CASES = None


def vertical():
    """(z, the 200 cells of rows 50..249 beside the trough's axis): synthetic_channel(300, theta=0) - the trough runs along a
    column, the profiles along the rows (orientation 0), t = de row.  Every cell lies up to one column off the axis."""
    z = cr.channel_z(N, theta=0.0, f0=float(cr.freqs_of_sigma([4.0])[0]))
    x = np.linspace(-N / 2, N / 2, num=N)
    col = int(np.argmin(np.abs(x)))
    off = np.random.default_rng(11).integers(-1, 2, 200)
    return z, np.arange(50, 250, dtype=np.int64) * N + col + off


def gpu_cases():
    """The cases as dicts: name, z, de, cells (int64), labels (one per cell), angle (one per cell), h, w, D, frequencies,
    window, step, delta, min_samples, min_profiles; 'stage' names the cells of cases that share them.  Every case runs in
    both modes.  DEMs are 96 x 128 or 300 x 300 but for the 64 frequencies at h = 100 (256 x 256).  Seeded: the same on every
    box."""
    global _CASES
    if _CASES is not None:
        return _CASES
    cases = []

    def add(name, z, de, cells, labels, angle, h, w, D, freqs, window, step, delta=1.0, ms=4, mp=1, stage=None):
        cells = np.ascontiguousarray(cells, dtype=np.int64)
        angle = np.ascontiguousarray(np.broadcast_to(np.asarray(angle, dtype=np.float64), cells.shape))
        cases.append(dict(name=name, stage=stage or name, z=z, de=float(de), cells=cells,
                          labels=np.ascontiguousarray(np.broadcast_to(np.asarray(labels, dtype=np.int64), cells.shape)), angle=angle,
                          h=h, w=w, D=D, frequencies=np.ascontiguousarray(freqs, dtype=np.float64), window=float(window),
                          step=float(step), delta=delta, min_samples=ms, min_profiles=mp))

    rng = np.random.default_rng(20261021)
    # 1. the boundaries of the runs of 64: strike_reference.RUNS' (window, step) on 200 cells of one column; short profiles
    zv, col = vertical()
    f4 = cr.freqs_of_sigma(np.geomspace(2.0, 8.0, 4))
    for count, (window, step) in stk.RUNS.items():
        add("run %d" % count, zv, 1.0, col, 4, 0.0, 8, 1, 2, f4, window, step, stage="vertical")
    # 2. unusable profiles: rows 60 and 63 are NaN (w = 0: their cells have no profile) in the middle of a window's run, rows
    # 100..120 leave windows without a usable profile and, at their ends, with one or two; the reach has no cell in rows
    # 140..169: empty windows.  A second reach runs down the right edge, its profiles clipped.  A third is one cell of a row
    # that is NaN but for what leaves it the four points j = -3, -2, 1, 2 (a sample reads its right-hand neighbour, with
    # weight 0): dof < 1 at min_samples 2
    zn = zv.copy()
    zn[[60, 63], :] = np.nan
    zn[100:121, :] = np.nan
    zn[270, :] = np.nan
    zn[270, 147:150] = zv[270, 147:150]
    zn[270, 151:154] = zv[270, 151:154]
    keep = np.r_[0:90, 120:200]                                           # rows 50..139 and 170..249
    edge = np.arange(30, 70, dtype=np.int64) * N + (N - 1 - (np.arange(40) % 8))
    perm = rng.permutation(len(keep) + len(edge) + 1)
    un = (np.concatenate([col[keep], edge, [270 * N + 150]])[perm], np.repeat([3, 7, 9], [len(keep), len(edge), 1])[perm], 0.0)
    add("unusable", zn, 1.0, *un, 8, 0, 2, f4, 10, 5, ms=2, stage="unusable")
    add("unusable min_profiles 3", zn, 1.0, *un, 8, 0, 2, f4, 10, 5, ms=2, mp=3, stage="unusable")
    # 3. the lanes and where the table sits: channel_segment_reference's small trough, 4 cells wide, theta = 0.2
    f0 = float(cr.freqs_of_sigma([4.0])[0])
    zs = cr.channel_z(128, ny=96, f0=f0)
    nx = zs.shape[1]

    def line(rows, off=3):
        rows = np.asarray(rows)
        return cr.line_cells(128, 96, rows) + rng.integers(-off, off + 1, len(rows))

    on = line(np.arange(24, 72, 2))
    ang = 0.2 + 0.05 * rng.standard_normal(len(on))
    lab2 = np.repeat([2, 1], [14, 10])
    add("F = 1", zs, 1.0, on, lab2, ang, 20, 2, 3, [f0], 12, 6)
    zb = cr.channel_z(256, f0=float(cr.freqs_of_sigma([6.0])[0]))
    mid = cr.line_cells(256, 256, np.arange(110, 146, 3)) + rng.integers(-3, 4, 12)
    add("F = 64, h = 100, D = 8", zb, 1.0, mid, np.repeat([2, 1], [7, 5]), 0.2, 100, 1, 8,
        cr.freqs_of_sigma(np.geomspace(0.5, 50.0, 64)), 12, 6)
    add("D = 0", zs, 1.0, on, lab2, ang, 30, 2, 0, cr.freqs_of_sigma(np.geomspace(0.5, 15.0, 12)), 12, 6)
    add("D = h - min_samples", zs, 1.0, on, lab2, ang, 12, 1, 8, cr.freqs_of_sigma(np.geomspace(0.7, 6.0, 10)), 12, 6)
    add("de = 2", zs, 2.0, on, lab2, ang, 30, 5, 4, cr.freqs_of_sigma(2.0 * np.geomspace(1.0, 14.0, 12)), 24, 12, delta=2.0)
    # 4. several reaches: strikes near 0.2 (twice) and a vertical one, one cell alone; labels not consecutive, labels <= 0
    # mixed in; shuffled
    across = int(np.median(cr.line_cells(128, 96, np.arange(20, 50)) % nx))          # a column the trough crosses in rows 20..49
    parts = [line(np.arange(14, 40)), line(np.arange(44, 70)), line([76]), np.arange(20, 50) * nx + across, line(np.arange(15, 25))]
    lab = np.repeat([5, 2, 11, 9, 0], [len(p) for p in parts])
    lab[-3:] = [-1, 0, -4]
    a5 = np.repeat([0.2, 0.2, 0.2, 0.0, 0.2], [len(p) for p in parts]) + 0.02 * rng.standard_normal(len(lab))
    perm = rng.permutation(len(lab))
    add("several reaches", zs, 1.0, np.concatenate(parts)[perm], lab[perm], a5[perm], 20, 1, 3,
        cr.freqs_of_sigma(np.geomspace(0.8, 10.0, 8)), 10, 5)
    # 5. NaN holes: scattered, so that a window holds complete and incomplete profiles - both routes of the search in one sum
    zh = zs.copy()
    zh[rng.random(zh.shape) < 0.004] = np.nan
    add("NaN holes", zh, 1.0, line(np.arange(20, 76, 2)), 6, 0.2 + 0.05 * rng.standard_normal(28), 20, 0, 3,
        cr.freqs_of_sigma(np.geomspace(0.5, 10.0, 12)), 16, 8, ms=6)
    # 6. a hole at the centre at pi f de = 6 (channel_segment_reference's layout): a hole over j = -3..3 of the profile of row
    # 40 leaves that frequency dead in it, and so in every window that holds it; the other windows keep it
    zd = zs.copy()
    zd[40, 57:64] = np.nan
    hole = np.array([44 * nx + 60, 40 * nx + 60, 48 * nx + 61, 52 * nx + 61, 56 * nx + 62, 60 * nx + 62])
    add("a hole at the centre at pi f de = 6", zd, 1.0, hole, 1, 0.0, 20, 0, 0,
        np.concatenate([cr.freqs_of_sigma(np.geomspace(1.0, 8.0, 7)), [6.0 / np.pi]]), 8, 4)
    add("every frequency dead", zd, 1.0, hole, 1, 0.0, 20, 0, 0, [6.0 / np.pi], 8, 4)
    _CASES = cases
    return cases
