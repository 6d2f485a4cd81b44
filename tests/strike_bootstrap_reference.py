"""numpy restatement of sc_strike_bootstrap / sl.bootstrap_along_strike (docs/strike.md, "Intervals per station"), written
from the definition.  The hand-over and the windows are ``strike_reference``'s (cut cell by cell, never by a search in a
sorted array); the blocks of a window are cut by a plain loop over its cells; the per-profile terms, the sums in runs of
64, the replicate's argmax and the rank rule are ``bootstrap_reference``'s (projection by a QR, never the device's
passes); the draws are uint64 numpy arithmetic with the station in the key."""
import math

import numpy as np

import bootstrap_reference as br
import strike_reference as stk

NEAR, RTOL = br.NEAR, br.RTOL
U = np.uint64
ROW_INTS = ("label", "station", "n_cells", "n_profiles", "n_blocks", "replicates")
ROW_FLOATS = ("kt0", "kt_lo", "kt_hi", "a0", "a_mean", "a_sd", "a_lo", "a_hi")


def draws(seed, label, station, R, nb):
    """(R, nb) int64: the block of draw k of replicate r = 1..R, for window ``station`` of the segment ``label``."""
    key = br.mix(np.array([seed], dtype=U) ^ (np.array([label], dtype=U) * U(0x9E3779B97F4A7C15))
                 ^ (np.array([station], dtype=U) * U(0xD1B54A32D192ED03)))
    r = np.arange(1, R + 1, dtype=U)[:, None]
    k = np.arange(nb, dtype=U)[None, :]
    u = br.mix(key + ((r << U(32)) | k))
    return (((u >> U(32)) * U(nb)) >> U(32)).astype(np.int64)


def blocks(t, block_length):
    """The blocks of a window whose cells lie at ``t`` (ascending): a list of (first, end) ranges of its cells, one per
    block that holds a cell - a plain loop."""
    out, cur = [], None
    for i, v in enumerate(t):
        b = int(math.floor((v - t[0]) / block_length))
        if b != cur:
            out.append([i, i + 1])
            cur = b
        else:
            out[-1][1] = i + 1
    return [tuple(r) for r in out]


def bootstrap_window(terms, tw, label, station, A, ages, block_length, R, level, seed, min_profiles, min_blocks):
    """One window's row as a dict: the fields of sc_strike_boot, plus 'index' and 'a' (R + 1, replicate 0 first), 'near'
    (R + 1 bools) and 'hist' (A).  ``terms``: per cell of the window in hand-over order, (usable, See, Sep)."""
    blk = blocks(tw, block_length)
    nb = len(blk)
    T = np.zeros((nb, A, 2))
    m = 0
    for g, (c0, c1) in enumerate(blk):
        rows = [np.stack([See, Sep], axis=1) for ok, See, Sep in terms[c0:c1] if ok]
        m += len(rows)
        if rows:
            T[g] = br.run_sum(rows)
    row = {"label": int(label), "station": int(station), "n_cells": len(tw), "n_profiles": m, "n_blocks": nb, "replicates": R,
           "n_failed": 0, "kt_index0": -1, "lo_index": -1, "hi_index": -1, "status": 1, "index": np.full(R + 1, -1),
           "a": np.full(R + 1, np.nan), "near": np.zeros(R + 1, dtype=bool), "hist": np.zeros(A, dtype=np.int64), "terms": T}
    for f in ROW_FLOATS:
        row[f] = np.nan
    if nb < min_blocks or m < min_profiles:
        return row
    picks = np.concatenate([np.arange(nb)[None, :], draws(seed, label, station, R, nb)])
    for r in range(R + 1):
        row["index"][r], row["a"][r], row["near"][r] = br.replicate(T, picks[r])
    ok = row["index"][1:] >= 0
    n_ok = int(ok.sum())
    row["n_failed"] = R - n_ok
    row["hist"] = np.bincount(row["index"][1:][ok], minlength=A)
    if n_ok == 0:
        return row
    klo, khi = br.ranks(n_ok, level)
    x = np.sort(row["index"][1:][ok])
    av = row["a"][1:][ok]
    xs = np.sort(av)
    lo, hi = int(x[klo]), int(x[khi])
    i0 = int(row["index"][0])
    row.update(kt_index0=i0, lo_index=lo, hi_index=hi, status=(2 if lo == 0 else 0) + (4 if hi == A - 1 else 0),
               kt0=float(ages[i0]) if i0 >= 0 else np.nan, kt_lo=float(ages[lo]), kt_hi=float(ages[hi]), a0=float(row["a"][0]),
               a_mean=float(av.mean()), a_sd=float(av.std(ddof=1)) if n_ok > 1 else np.nan, a_lo=float(xs[klo]),
               a_hi=float(xs[khi]))
    return row


def bootstrap_along_strike(z, de, cells, labels, angle, h, w, ages, window, step, block_length, R, level=0.95, seed=0, D=0,
                           min_samples=4, min_profiles=1, min_blocks=5):
    """Rows (a list of dicts, one per (label, station) in that order): ``bootstrap_window``'s, plus 't', 'row', 'col'
    and 'where' (the input positions of the window's cells in hand-over order)."""
    z = np.asarray(z, dtype=np.float64)
    ages = np.asarray(ages, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.int64)
    angle = np.broadcast_to(np.asarray(angle, dtype=np.float64), (len(cells),))
    sa, ca = np.sin(angle), np.cos(angle)
    nx, A = z.shape[1], len(ages)
    cache = {}

    def terms_of(c):                                                     # (a cell lies in several windows)
        if c not in cache:
            cache[c] = br.profile_terms(z, de, cells[c], sa[c], ca[c], h, w, D, ages, min_samples)[:3]
        return cache[c]
    rows = []
    for L, pos, t, _ in stk.handover(cells, labels, angle, nx, de):
        centres, ranges = stk.stations(t, window, step)
        for k, (u, (lo, hi)) in enumerate(zip(centres, ranges)):
            wp = pos[lo:hi]
            row = bootstrap_window([terms_of(int(c)) for c in wp], t[lo:hi], L, k, A, ages, float(block_length), R, level,
                                   seed, min_profiles, min_blocks)
            row.update(t=u, where=wp, row=float(np.mean(cells[wp] // nx)) if len(wp) else np.nan,
                       col=float(np.mean(cells[wp] % nx)) if len(wp) else np.nan)
            rows.append(row)
    return rows


def compare(ref, table, hist):
    """The device's rows and (NW, A) histograms against ``ref``.  The integers and the histograms match exactly, but for
    a window that holds a replicate whose two largest Q_i the restatement finds within NEAR: such replicates may be at
    most 0.1 % of all (bootstrap_reference.compare's cap), and of such a window only what no replicate decides is
    compared.  The floats agree to RTOL.  Returns the figures."""
    out = {"windows": len(ref), "booted": 0, "replicates": 0, "near": 0, "skipped": 0, "a": 0.0}
    assert len(table) == len(ref) and hist.shape[0] == len(ref)
    for s, (r, g) in enumerate(zip(ref, table)):
        key = (r["label"], r["station"])
        for f in ROW_INTS:
            assert int(g[f]) == r[f], (key, f, g[f], r[f])
        assert abs(float(g["t"]) - r["t"]) <= 1e-12 * max(1.0, abs(r["t"])), (key, g["t"], r["t"])
        for f in ("row", "col"):
            assert (np.isnan(g[f]) and np.isnan(r[f])) or abs(float(g[f]) - r[f]) <= 1e-12 * max(1.0, abs(r[f])), (key, f)
        if r["status"] == 1 and not r["near"].any():
            assert int(g["status"]) == 1 and int(g["n_failed"]) == r["n_failed"], (key, g["status"], g["n_failed"])
            for f in ("kt_index0", "lo_index", "hi_index"):
                assert int(g[f]) == -1, (key, f)
            for f in ROW_FLOATS + ("height0", "height_lo", "height_hi"):
                assert np.isnan(g[f]), (key, f)
            assert not hist[s].any(), key
            continue
        out["booted"] += 1
        out["replicates"] += r["replicates"] + 1
        out["near"] += int(r["near"].sum())
        assert int(hist[s].sum()) == r["replicates"] - int(g["n_failed"]), key
        if r["near"].any():
            out["skipped"] += 1
            continue
        assert int(g["n_failed"]) == r["n_failed"] and np.array_equal(hist[s], r["hist"]), (key, hist[s], r["hist"])
        for f in ("kt_index0", "lo_index", "hi_index", "status"):
            assert int(g[f]) == r[f], (key, f, g[f], r[f])
        for f in ("kt0", "kt_lo", "kt_hi"):
            assert float(g[f]) == r[f], (key, f)
        for f in ("a0", "a_mean", "a_sd", "a_lo", "a_hi"):
            if np.isnan(r[f]):
                assert np.isnan(g[f]), (key, f)
                continue
            # (a_sd is formed from the differences v_r - a_mean, each rounded at eps |a_mean|: where every replicate has
            # the same a - two blocks, one of them without a profile - it is that rounding and nothing else, 0 here or
            # there, and is held against a_mean)
            scale = abs(r["a_mean"]) if f == "a_sd" and abs(r[f]) <= 1e-12 * abs(r["a_mean"]) else abs(r[f])
            d = abs(float(g[f]) - r[f]) / scale
            assert d <= RTOL, (key, f, g[f], r[f])
            out["a"] = max(out["a"], d)
        assert float(g["height0"]) == 2.0 * float(g["a0"]) and float(g["height_lo"]) == 2.0 * float(g["a_lo"])
        assert float(g["height_hi"]) == 2.0 * float(g["a_hi"])
    assert out["near"] <= 1e-3 * max(1, out["replicates"]), out
    return out


# ---- the inputs of tests/test_gpu_strike_bootstrap.py -----------------------------------------------------------------------
N, H = stk.N, 20
RUNS = (1, 63, 64, 65, 129)          # usable profiles of the first block of the five segments of "runs"
RUN_ROWS = 26                        # rows of that block, five cells a row


def run_cells():
    """(cells, labels) of "runs": segment c of RUNS (label its position + 1) has c cells in the rows 60..85, five a row in
    the columns around the scarp's, row by row - one block of 26 - and three cells in row 86, the second block."""
    _, col = stk.vertical()
    c0 = int(col[0] % N)
    grid = np.array([r * N + c0 + d for r in range(60, 60 + RUN_ROWS) for d in (-2, -1, 0, 1, 2)], dtype=np.int64)
    tail = np.array([(60 + RUN_ROWS) * N + c0 + d for d in (-1, 0, 1)], dtype=np.int64)
    cells = np.concatenate([np.concatenate([grid[:c], tail]) for c in RUNS])
    return cells, np.repeat(np.arange(1, len(RUNS) + 1), [c + 3 for c in RUNS])


def gpu_cases():
    """The cases as dicts: name, z, cells, labels, angle (one per cell), h, w (cells), ages, window, step, block_length,
    R, level, seed, min_blocks, min_profiles, min_samples, D - all at de = 1.  Seeded: the same on every box."""
    five = [3.0, 6.0, 10.0, 18.0, 30.0]
    cases = []

    def add(name, z, cells, labels, angle, window, step, bl, h=H, w=1, kt=five, R=100, level=0.95, seed=7, mb=5, mp=1, ms=4, D=0):
        cells = np.ascontiguousarray(cells, dtype=np.int64)
        angle = np.ascontiguousarray(np.broadcast_to(np.asarray(angle, dtype=np.float64), cells.shape))
        cases.append(dict(name=name, z=z, cells=cells, labels=np.asarray(labels, dtype=np.int64), angle=angle, h=h, w=w,
                          ages=np.asarray(kt, dtype=np.float64), window=float(window), step=float(step), block_length=float(bl),
                          R=R, level=level, seed=seed, min_blocks=mb, min_profiles=mp, min_samples=ms, D=D))

    zv, col = stk.vertical()
    lab = np.full(200, 4)
    # 1. blocks of 1, 63, 64, 65 and 129 usable profiles: the boundaries of the runs of 64.  One window per segment
    rc, rl = run_cells()
    add("runs", zv, rc, rl, 0.0, 60, 60, RUN_ROWS, mb=2)
    # 2. 200 cells of one column, t = row: windows of about 31 cells, blocks of 3 rows
    for R in (1, 1000, 4096):
        add("R %d" % R, zv, col, lab, 0.0, 30, 15, 3, R=R)
    add("one age", zv, col, lab, 0.0, 30, 15, 3, kt=[10.0])
    add("64 ages", zv, col, lab, 0.0, 30, 15, 3, kt=10 ** np.linspace(0, 1.6, 64))
    add("level 0.5", zv, col, lab, 0.0, 30, 15, 3, level=0.5)
    add("level 0.999", zv, col, lab, 0.0, 30, 15, 3, level=0.999)
    # 3. more than 64 blocks: eight ages, blocks of one cell, the middle window of 70 cells - a second batch of draws
    add("70 blocks", zv, col, lab, 0.0, 69, 69, 1, kt=10 ** np.linspace(0.3, 1.5, 8))
    # 4. window 10 at step 7 in blocks of 2: the windows hold 11 or 10 cells in five blocks, those at the segment's ends 8
    # cells in four: min_blocks and one fewer
    add("min_blocks", zv, col, lab, 0.0, 10, 7, 2, mb=5)
    # 5. a hole longer than the window: empty windows
    keep = np.r_[0:90, 120:200]
    add("a hole", zv, col[keep], lab[keep], 0.0, 10, 5, 2, mb=3)
    # 6. two blocks, the second on NaN ground (w = 0: its cells have no profile): a replicate that draws it twice fails
    zn = zv.copy()
    zn[55:60, :] = np.nan
    add("a NaN block", zn, col[:10], np.full(10, 6), 0.0, 20, 20, 5, w=0, mb=2)
    # 7. several segments - strikes 0.2 (twice), a diagonal, one cell; labels not consecutive; shuffled - and the shift
    import profile_reference as pr
    rng = np.random.default_rng(20261022)
    zs = pr.synthetic_z(N, sigma=0.3, theta=0.2, seed=6)
    d = np.arange(100, 140, dtype=np.int64)
    parts = [stk.line_cells(np.arange(40, 100)), d * N + d, stk.line_cells([145]), stk.line_cells(np.arange(150, 221))]
    sl_ = np.repeat([5, 2, 11, 9], [len(p) for p in parts])
    ang = np.repeat([0.2, np.pi / 4, 0.2, 0.2], [len(p) for p in parts]) + 0.02 * rng.standard_normal(len(sl_))
    perm = rng.permutation(len(sl_))
    add("several segments", zs, np.concatenate(parts)[perm], sl_[perm], ang[perm], 24, 8, 3, mb=4)
    off = rng.integers(-2, 3, 60)
    add("D 3", zs, stk.line_cells(np.arange(60, 120)) + off, np.full(60, 8), 0.2, 24, 12, 3, mb=4, D=3)
    return cases


def restate(case):
    return bootstrap_along_strike(case["z"], 1.0, case["cells"], case["labels"], case["angle"], case["h"], case["w"],
                                  case["ages"], case["window"], case["step"], case["block_length"], case["R"], case["level"],
                                  case["seed"], case["D"], case["min_samples"], case["min_profiles"], case["min_blocks"])


# ---- the recovery case of docs/strike.md ------------------------------------------------------------------------------------
def taper_case(n=300, sigma=0.3, seed=11):
    """(z, cells, planted): synthetic_scarp's surface with the scarp along a column (theta = 0) and an amplitude that
    tapers linearly along the strike, 1 at row 50 to 0.2 at row 249, under noise; the 200 cells of rows 50..249 in the
    scarp's column; ``planted``: the offset 2 a of every row."""
    from scipy.special import erf
    x = np.linspace(-n / 2, n / 2, num=n)
    rows = np.arange(n, dtype=np.float64)
    amp = np.clip(1.0 - 0.8 * (rows - 50.0) / 199.0, 0.2, 1.0)
    yrot = -x[None, :] * np.ones((n, 1))
    z = -amp[:, None] * erf(yrot / (2.0 * np.sqrt(10.0))) + 0.01 * yrot
    z = z + sigma * np.random.default_rng(seed).standard_normal((n, n))
    z = z.astype(np.float32).astype(np.float64)
    col = int(np.argmin(np.abs(x)))
    return z, np.arange(50, 250, dtype=np.int64) * n + col, 2.0 * amp


TAPER = dict(h=20, w=1, window=30.0, step=10.0, block_length=3.0, R=500, level=0.95, seed=3, min_blocks=5)


def taper_counts(rows, planted):
    """(stations, those whose [height_lo, height_hi] holds the planted offset at the station, those whose point estimate
    height0 lies within 5 % of it): the planted offset is linear along the strike, so at a station it is the value at
    ``t``, interpolated between the rows."""
    booted = [r for r in rows if int(r["status"]) != 1]
    at = [float(np.interp(float(r["t"]), np.arange(len(planted), dtype=np.float64), planted)) for r in booted]
    inside = sum(2.0 * float(r["a_lo"]) <= p <= 2.0 * float(r["a_hi"]) for r, p in zip(booted, at))
    point = sum(abs(2.0 * float(r["a0"]) - p) <= 0.05 * p for r, p in zip(booted, at))
    return len(booted), int(inside), int(point)
