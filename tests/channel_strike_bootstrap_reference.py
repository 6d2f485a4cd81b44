"""numpy restatement of sc_channel_strike_bootstrap / sl.bootstrap_channels_along_strike (docs/channels.md, "Intervals per
station"), built from the existing ones.  The hand-over and the windows are ``channel_strike_reference.handover``; the
per-profile terms ``channel_bootstrap_reference.stage_of`` (a float64 ``lstsq`` for each cell, frequency and shift, See and
Sep by projection - never the device's passes); the blocks of a window ``strike_bootstrap_reference.blocks``, a plain loop
over its cells' along-strike coordinates; the draws ``strike_bootstrap_reference.draws``, uint64 numpy arithmetic with the
station in the key; the replicates ``channel_bootstrap_reference.replicates``, in float64 or in ``np.longdouble`` for the
reference-side noise floor; the run sum and the rank rule ``bootstrap_reference``'s."""
import math

import numpy as np

import bootstrap_reference as br
import channel_bootstrap_reference as cb
import channel_reference as cr
import channel_segment_reference as csr
import channel_strike_reference as cw
import strike_bootstrap_reference as sbr

NEAR, RTOL = cb.NEAR, cb.RTOL
MODES = cb.MODES
ROW_INTS = ("label", "station", "n_cells", "n_profiles", "n_blocks", "replicates")
ROW_FLOATS = cb.ROW_FLOATS
DERIVED = cb.DERIVED


# ---- one window -----------------------------------------------------------------------------------------------------------------
def bootstrap_window(terms, tw, label, station, freqs, mode, block_length, R, level, seed, min_profiles, min_blocks,
                     dtype=np.float64):
    """One window's row as a dict from its cells' stage-one terms in hand-over order (None: not usable) and their
    along-strike coordinates ``tw``: the fields of sc_channel_strike_boot, plus 'index' and 'a' (R + 1, replicate 0 first),
    'near', 'n_live', 'hist', 'terms' (nb, F, 2) and 'mb'."""
    F = len(freqs)
    blk = sbr.blocks(tw, block_length)
    nb = len(blk)
    cols = (2, 3) if mode == "segment" else (0, 1)
    T, mb = np.zeros((nb, F, 2)), np.zeros(nb, dtype=np.int64)
    for g, (c0, c1) in enumerate(blk):
        rows = [t[:, cols] for t in terms[c0:c1] if t is not None]
        mb[g] = len(rows)
        if rows:
            T[g] = br.run_sum(rows)
    m = int(mb.sum())
    row = {"label": int(label), "station": int(station), "n_cells": len(tw), "n_profiles": m, "n_blocks": nb, "replicates": R,
           "n_failed": 0, "f_index0": -1, "lo_index": -1, "hi_index": -1, "status": 1, "index": np.full(R + 1, -1),
           "a": np.full(R + 1, np.nan), "near": np.zeros(R + 1, dtype=bool), "n_live": np.zeros(R + 1, dtype=np.int64),
           "hist": np.zeros(F, dtype=np.int64), "terms": T, "mb": mb}
    for f in ROW_FLOATS:
        row[f] = np.nan
    if nb < min_blocks or m < min_profiles:
        return row
    picks = np.concatenate([np.arange(nb, dtype=np.int64)[None, :], sbr.draws(seed, label, station, R, nb)])
    row["index"], row["a"], row["near"], row["n_live"] = cb.replicates(T, mb, picks, mode, dtype)
    ok = row["index"][1:] >= 0
    n_ok = int(ok.sum())
    row["n_failed"] = R - n_ok
    row["hist"] = np.bincount(row["index"][1:][ok], minlength=F)
    if n_ok == 0:
        row["status"] = 1 | 32 if row["index"][0] < 0 else 1
        return row
    klo, khi = br.ranks(n_ok, level)
    x = np.sort(row["index"][1:][ok])
    av = row["a"][1:][ok]
    ar = cb.area_of(av, freqs[row["index"][1:][ok]].astype(dtype))
    lo, hi = int(x[klo]), int(x[khi])
    i0 = int(row["index"][0])
    row.update(f_index0=i0, lo_index=lo, hi_index=hi, status=(2 if lo == 0 else 0) + (4 if hi == F - 1 else 0),
               f0=float(freqs[i0]) if i0 >= 0 else np.nan, f_lo=float(freqs[lo]), f_hi=float(freqs[hi]),
               a0=row["a"][0], area0=cb.area_of(row["a"][0], freqs[i0]) if i0 >= 0 else np.nan)
    for name, v in (("a", av), ("area", ar)):
        mean = cb.seq_sum(v) / n_ok
        row[name + "_mean"] = mean
        row[name + "_sd"] = np.sqrt(cb.seq_sum((v - mean) ** 2) / (n_ok - 1)) if n_ok > 1 else np.nan
        vs = np.sort(v)
        row[name + "_lo"], row[name + "_hi"] = vs[klo], vs[khi]
    return row


_ROWS = {}


def restate(case, mode, longdouble=False):
    """The restatement's rows of a case, one per (label, station) in that order: bootstrap_window's, plus 't', 'row', 'col'
    and 'where' (the input positions of the window's cells in hand-over order)."""
    key = (case["name"], mode, longdouble, case["seed"])
    if key in _ROWS:
        return _ROWS[key]
    terms = cb.stage_of(case)
    nx = case["z"].shape[1]
    lab, order, sws, lo, hi, centre = cw.handover(case)
    _, groups = csr.group(case["labels"])
    rows = []
    for s, L in enumerate(lab):
        a = br.strike_of(case["angle"][groups[s]])
        for g in range(int(sws[s]), int(sws[s + 1])):
            wp = order[lo[g]:hi[g]]
            tw = [case["de"] * (float(c // nx) * math.cos(a) + float(c % nx) * math.sin(a)) for c in case["cells"][wp]]
            assert all(u <= v for u, v in zip(tw, tw[1:]))                  # (the hand-over is sorted along the strike)
            row = bootstrap_window([terms[k] for k in wp], tw, L, g - int(sws[s]), case["frequencies"], mode,
                                   case["block_length"], case["R"], case["level"], case["seed"], case["min_profiles"],
                                   case["min_blocks"], np.longdouble if longdouble else np.float64)
            row.update(t=float(centre[g]), where=wp, row=float(np.mean(case["cells"][wp] // nx)) if len(wp) else np.nan,
                       col=float(np.mean(case["cells"][wp] % nx)) if len(wp) else np.nan)
            rows.append(row)
    _ROWS[key] = rows
    return rows


# ---- comparing the device's table with the restatement -----------------------------------------------------------------------
def sd_rounding(rows):
    """(label, station, field) of every standard deviation of the restatement's rows that lies below 1e-12 of its mean."""
    return [(r["label"], r["station"], k + "_sd") for r in rows if not r["status"] & 1 for k in ("a", "area")
            if not np.isnan(float(r[k + "_sd"])) and abs(float(r[k + "_sd"])) <= 1e-12 * abs(float(r[k + "_mean"]))]


def compare(ref, table, hist):
    """The device's rows and (NW, F) histograms against ``ref``.  The integers and the histograms match exactly, but for a
    window that holds a replicate whose two best keys the restatement finds within NEAR: such replicates may be at most
    0.1 % of all, none of them replicate 0, and of such a window only what no replicate decides is compared.  The floats -
    the two standard deviations like the others - are within RTOL of their own size; an sd that the restatement finds
    below 1e-12 of its mean - every replicate has the same value - is rounding alone and is held against the mean.  Returns
    the figures."""
    out = {"windows": len(ref), "booted": 0, "replicates": 0, "near": 0, "skipped": 0, "a": 0.0, "sd": 0.0}
    assert len(table) == len(ref) and hist.shape[0] == len(ref)
    for s, (r, g) in enumerate(zip(ref, table)):
        key = (r["label"], r["station"])
        for f in ROW_INTS:
            assert int(g[f]) == r[f], (key, f, g[f], r[f])
        assert abs(float(g["t"]) - r["t"]) <= 1e-12 * max(1.0, abs(r["t"])), (key, g["t"], r["t"])
        for f in ("row", "col"):
            assert (np.isnan(g[f]) and np.isnan(r[f])) or abs(float(g[f]) - r[f]) <= 1e-12 * max(1.0, abs(r[f])), (key, f)
        assert not r["near"][0], (key, "a near-tie at replicate 0")
        out["near"] += int(r["near"].sum())
        if r["status"] & 1 and not r["near"].any():
            assert int(g["status"]) == r["status"] and int(g["n_failed"]) == r["n_failed"], (key, g["status"], g["n_failed"])
            for f in ("f_index0", "lo_index", "hi_index"):
                assert int(g[f]) == -1, (key, f)
            for f in ROW_FLOATS + DERIVED:
                assert np.isnan(g[f]), (key, f)
            assert not hist[s].any(), key
            continue
        out["booted"] += 1
        out["replicates"] += r["replicates"] + 1
        assert int(hist[s].sum()) == r["replicates"] - int(g["n_failed"]), key
        if r["near"].any():
            out["skipped"] += 1
            continue
        assert int(g["n_failed"]) == r["n_failed"] and np.array_equal(hist[s], r["hist"]), (key, hist[s], r["hist"])
        for f in ("f_index0", "lo_index", "hi_index", "status"):
            assert int(g[f]) == r[f], (key, f, g[f], r[f])
        for f in ("f0", "f_lo", "f_hi"):
            assert float(g[f]) == r[f] or (np.isnan(g[f]) and np.isnan(r[f])), (key, f)
        for f in ROW_FLOATS[3:]:
            want = float(r[f])
            if np.isnan(want):
                assert np.isnan(g[f]), (key, f)
                continue
            # (an sd is formed from the differences v_r - mean, each rounded at eps |mean|: where every replicate has the same
            # value it is that rounding and nothing else, 0 here or there, and is held against the mean:
            # strike_bootstrap_reference.compare's rule.  ONE window of the cases needs it, in both modes: "empty windows",
            # label 3, station 10 - three blocks of 2, 0 and 0 usable profiles beside the NaN rows, so every replicate that
            # does not fail has the first block's a: a_sd is 1.3e-15 of an a_mean of -1.0.  sd_rounding() finds such rows
            # and tests/test_channel_strike_bootstrap_host.py pins that there is no other)
            scale = abs(want)
            if f.endswith("_sd") and abs(want) <= 1e-12 * abs(float(r[f[:-2] + "mean"])):
                scale = abs(float(r[f[:-2] + "mean"]))
            d = abs(float(g[f]) - want) / scale if scale != 0.0 else (0.0 if float(g[f]) == 0.0 else np.inf)
            assert d <= RTOL, (key, f, g[f], want)
            out["a"] = max(out["a"], d)
            if f.endswith("_sd"):
                out["sd"] = max(out["sd"], d)
        # what Python adds: fit_channels' formulas
        i0 = r["f_index0"]
        assert float(g["depth_lo"]) == -float(g["a_hi"]) and float(g["depth_hi"]) == -float(g["a_lo"])
        if i0 >= 0:
            want = cr.derived(float(g["f0"]), float(g["f_lo"]), float(g["f_hi"]), float(g["a0"]))
            for f, w in (("depth0", "depth"), ("sigma0", "sigma"), ("width0", "width"), ("width_lo", "width_lo"),
                         ("width_hi", "width_hi"), ("curvature0", "curvature")):
                assert np.isclose(float(g[f]), want[w], rtol=1e-14, atol=0.0), (key, f)
            assert float(g["area0"]) == cb.area_of(float(g["a0"]), float(g["f0"])), key
    assert out["near"] <= 1e-3 * max(1, out["replicates"]), out
    return out


# ---- the inputs of tests/test_gpu_channel_strike_bootstrap.py ----------------------------------------------------------------------
N, H = cb.N, cb.H
RUNS = (63, 64, 65, 130)             # usable profiles of the first block of the reaches of the two "run" cases
RUN_ROWS = 26                        # rows of that block, five cells a row
NAMES = ["nb 1 4 5 70", "R 1", "R 1000", "R 4096", "level 0.5", "level 0.999", "F 1", "F 64", "D 3", "runs 63 64 65", "run 130",
         "an empty block", "empty windows", "a dead frequency", "no live frequency", "several reaches", "caps"]
_CASES = None


def run_cells(counts):
    """(cells, labels): reach c of ``counts`` (label its position + 1) has c cells in the rows 40..65, five a row in the
    columns around the trough's line, row by row - at orientation 0 one block of 26 - and three cells in row 66, the second
    block."""
    rows = np.arange(40, 40 + RUN_ROWS)
    grid = (cb.line_cells(rows)[:, None] + np.arange(-2, 3)[None, :]).ravel()
    tail = cb.line_cells([40 + RUN_ROWS])[0] + np.arange(-1, 2)
    cells = np.concatenate([np.concatenate([grid[:c], tail]) for c in counts])
    return cells.astype(np.int64), np.repeat(np.arange(1, len(counts) + 1), [c + 3 for c in counts])


def gpu_cases():
    """The cases as dicts: channel_bootstrap_reference.gpu_cases' keys plus window and step.  Most are that list's cases -
    the same cells under the same 'stage' name, so one process forms their stage one once - with windows along the reach.
    DEMs are 160 x 160, h = 20, at most 300 cells.  Seeded: the same on every box."""
    global _CASES
    if _CASES is not None:
        return _CASES
    src = {c["name"]: c for c in cb.gpu_cases()}
    cases = []

    def add(name, of, window, step, bl, **kw):
        c = dict(src[of] if isinstance(of, str) else of, name=name, window=float(window), step=float(step), block_length=float(bl))
        c.update(kw)
        cases.append(c)

    base = src["nb 1 4 5 70"]
    # one window over every reach (the step is longer than the longest reach): reaches of 1, 4, 5 and 70 blocks, min_blocks 5
    add(NAMES[0], base, 200, 200, 1.5)
    # windows of 30 every 15 in blocks of 3: up to 30 cells in up to ten blocks; the short reaches have one window
    add(NAMES[1], base, 30, 15, 3, R=1)
    add(NAMES[2], base, 30, 15, 3, R=1000)
    add(NAMES[3], base, 30, 15, 3, R=4096)
    add(NAMES[4], base, 30, 15, 3, level=0.5)
    add(NAMES[5], base, 30, 15, 3, level=0.999)
    add(NAMES[6], "F 1", 30, 15, 3)
    add(NAMES[7], "F 64", 30, 15, 3)
    add(NAMES[8], "D 3", 30, 15, 3)
    # blocks of 63, 64, 65 and 130 usable profiles: the boundaries of the runs of 64.  Orientation 0: t = row
    z = base["z"]
    for name, counts in ((NAMES[9], RUNS[:3]), (NAMES[10], RUNS[3:])):
        rc, rl = run_cells(counts)
        add(name, dict(base, stage=name, cells=rc, labels=rl, angle=np.zeros(len(rc))), 60, 60, RUN_ROWS, min_blocks=2)
    # rows 66..93 are NaN: the cells of rows 76..83 have no usable profile.  Blocks of 3 put some of them in blocks of their
    # own inside windows of 30; windows of 6 hold cells and no usable profile, and where the reach has no cell - rows 100..111
    # are left out - no cell at all
    hole = src["an empty block"]
    add(NAMES[11], hole, 30, 15, 3)
    keep = (hole["cells"] // N < 100) | (hole["cells"] // N > 111)
    add(NAMES[12], dict(hole, stage="hole gap", cells=hole["cells"][keep], labels=hole["labels"][keep], angle=hole["angle"][keep]),
        6, 3, 2, min_blocks=2)
    # the frequency pi f de = 6 is dead in the profiles of rows 51..54 - the third of six blocks of the reach's one window -
    # and so in the replicates that draw it
    add(NAMES[13], "a dead frequency", 100, 100, 5)
    add(NAMES[14], "no live frequency", 100, 100, 5)
    # the four reaches of the base case as six: the two cells of reach 6 are reaches 11 and 12 of one cell each
    lab = base["labels"].copy()
    two = np.flatnonzero(lab == 6)
    lab[two] = [12, 11]
    add(NAMES[15], dict(base, labels=lab), 30, 15, 3)
    # the top of the range: R = 4096 at F = 64 with 64 blocks - 64 KiB of terms.  The first 64 rows of the long reach, one
    # block a row at block_length 1
    big = src["R 4096, F 64"]
    lab = big["labels"].copy()
    lab[(lab == 4) & (big["cells"] // N >= 25 + 64)] = 5
    add(NAMES[16], dict(big, labels=lab), 200, 200, 1.0)
    _CASES = cases
    return cases


# ---- the recovery of docs/channels.md, "Intervals per station" -----------------------------------------------------------------
# channel_bootstrap_reference's widening trough in the windows of "Width along a reach" - 60 every 30, eleven stations of 11
# to 20 profiles - in blocks of 9, three profiles each: 4 to 7 blocks a window, min_blocks 3
REC_WINDOW, REC_STEP, REC_BLOCK, REC_MIN_BLOCKS = cw.REC_WINDOW, cw.REC_STEP, 9.0, 3
REC_SPANS = (3, 0)
# ... [lo_index, hi_index] of the eleven stations as the restatement returns them (tests/test_channel_strike_bootstrap_host.py),
# in both depth modes
REC_INTERVALS = {3: [[15, 16], [15, 16], [15, 15], [14, 15], [14, 14], [13, 14], [12, 13], [12, 12], [11, 12], [10, 11], [10, 11]],
                 0: [[13, 13]] * 8 + [[13, 14], [13, 14], [13, 13]]}


def recovery(span):
    c = cb.widening_case(span)
    return dict(c, name="per station, " + c["name"], window=REC_WINDOW, step=REC_STEP, block_length=REC_BLOCK,
                min_blocks=REC_MIN_BLOCKS)
