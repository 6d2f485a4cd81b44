"""numpy restatement of sc_channel_bootstrap (docs/channels.md, "Intervals per reach"; include/scarplet_hip.h), written from
the definition.  Stage one is ``channel_segment_reference.stage_cell``: a float64 ``lstsq`` for EACH (cell, frequency, shift)
and the first smallest sse in the order tried; at the chosen shift ``sse*_ci`` and ``a_ci`` are that lstsq's, ``See_ci`` and
``Sep_ci`` come by projection (a QR of the columns 1 and s, never the device's passes).  The blocks, the strike, the run sum
and the rank rule are ``bootstrap_reference``'s, and so are the draws (``bootstrap_reference.draws`` forms them in uint64
arrays; the host test holds them against ``scarplet_amd.bootstrap.draw``).  A replicate's sums run over its drawn blocks one after
another in draw order - in float64, or in ``np.longdouble`` for the reference-side noise floor."""
import math

import numpy as np

import bootstrap_reference as br
import channel_reference as cr
import channel_segment_reference as csr

NEAR = 1e-12         # a replicate whose two best keys lie within this, relatively, may go either way
RTOL = br.RTOL       # floats against the device: the family's 1e-9
MODES = csr.MODES
ROW_INTS = ("label", "n_cells", "n_profiles", "n_blocks", "replicates")
ROW_FLOATS = ("f0", "f_lo", "f_hi", "a0", "a_mean", "a_sd", "a_lo", "a_hi", "area0", "area_mean", "area_sd", "area_lo", "area_hi")
DERIVED = ("depth0", "depth_lo", "depth_hi", "sigma0", "width0", "width_lo", "width_hi", "curvature0")
RPI = math.sqrt(np.pi)


def area_of(a, f):
    """channels._table's expression, in its order."""
    return -a / (RPI * f)


# ---- stage one ----------------------------------------------------------------------------------------------------------------
def profile_terms(c, de, freqs):
    """(F, 4) of a usable cell's stage-one record: sse*_ci, a_ci, See_ci, Sep_ci at d_ci; NaN where the frequency is dead."""
    F = len(freqs)
    out = np.full((F, 4), np.nan)
    s = c["j"].astype(np.float64) * de
    Q = np.linalg.qr(np.stack([np.ones_like(s), s], axis=1))[0]
    p2 = c["p"] - Q @ (Q.T @ c["p"])
    for i, f in enumerate(freqs):
        if np.isnan(c["curve"][i]):
            continue
        e = cr.gauss_column(c["j"], int(c["shifts"][i]), de, f)
        e2 = e - Q @ (Q.T @ e)
        out[i] = (c["curve"][i], c["coefs"][i, c["pick"][i], 2], e2 @ e2, e2 @ p2)
    return out


_STAGE = {}


def stage_of(case):
    """Per input cell of the case: None (label <= 0 or not usable) or profile_terms.  Kept under the case's 'stage' name:
    the cases that differ in the resampling alone share it."""
    if case["stage"] not in _STAGE:
        # (channel_segment_reference keeps its records by name: fit_channel_segments' restatement of the case finds them)
        cells = csr.stage_of(dict(case, name=case["stage"]))
        _STAGE[case["stage"]] = [profile_terms(c, case["de"], case["frequencies"]) if c is not None and c["usable"] else None
                                 for c in cells]
    return _STAGE[case["stage"]]


def pooled(case, mode):
    """fit_channel_segments' restatement (channel_segment_reference.restate) of the case's cells, on the shared stage one."""
    return csr.restate(dict(case, name=case["stage"], delta=case.get("delta", 1.0)), mode)


# ---- one reach ------------------------------------------------------------------------------------------------------------------
def picks_of(seed, label, R, nb):
    """(R + 1, nb): the blocks of every replicate in draw order, replicate 0 every block once."""
    return np.concatenate([np.arange(nb, dtype=np.int64)[None, :], br.draws(seed, label, R, nb)])


def replicates(T, mb, picks, mode, dtype=np.float64):
    """The replicates of one reach from its block terms T (nb, F, 2) and counts mb (nb), ``picks`` their drawn blocks: (index,
    -1 where failed; a; near: the two best keys within NEAR; the number of live frequencies), one entry per replicate.  The
    sums take the drawn blocks one after another."""
    n, nb = picks.shape
    F = T.shape[1]
    Tt = T.astype(dtype)
    acc = np.zeros((n, F, 2), dtype=dtype)
    M = np.zeros(n, dtype=np.int64)
    for k in range(nb):
        acc = acc + Tt[picks[:, k]]
        M = M + mb[picks[:, k]]
    X, Y = acc[..., 0], acc[..., 1]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if mode == "segment":
            Qv = Y * Y / X
            live = (X > 0) & np.isfinite(X) & ~np.isnan(Qv)
            key = -Qv
            val = Y / X
        else:
            live = (M > 0)[:, None] & ~np.isnan(X)
            key = X
            val = Y / M.astype(dtype)[:, None]
    key = np.where(live, key, np.inf)
    # the smallest key among the live ones, ties to the smaller index; a live +inf beats a frequency that is not live
    order = np.lexsort((np.arange(F)[None, :].repeat(n, 0), ~live, key), axis=1)
    best = order[:, 0]
    rows = np.arange(n)
    ok = live[rows, best]
    index = np.where(ok, best, -1)
    a = np.where(ok, val[rows, best], np.nan)
    near = np.zeros(n, dtype=bool)
    if F > 1:
        second = order[:, 1]
        k0, k1 = key[rows, best].astype(np.float64), key[rows, second].astype(np.float64)
        with np.errstate(invalid="ignore"):
            near = ok & live[rows, second] & (np.abs(k1 - k0) <= NEAR * np.abs(k0))
    return index, a, near, live.sum(axis=1)


def seq_sum(x):
    """The sum of a 1-D array in sequence from the first."""
    return np.add.accumulate(x)[-1]


def bootstrap_reach(terms, cells, label, nx, de, strike, freqs, mode, block_length, R, level, seed, min_profiles, min_blocks,
                    dtype=np.float64):
    """One reach's row as a dict from its cells' stage-one terms in input order: the fields of sc_channel_boot, plus 'index'
    and 'a' (R + 1, replicate 0 first), 'near', 'n_live', 'hist', 'terms' (nb, F, 2), 'mb' and 'picks'."""
    F = len(freqs)
    blk = br.blocks(cells, nx, de, strike, block_length)
    nb = len(blk)
    cols = (2, 3) if mode == "segment" else (0, 1)
    T, mb = np.zeros((nb, F, 2)), np.zeros(nb, dtype=np.int64)
    for g, pos in enumerate(blk):
        rows = [terms[k][:, cols] for k in pos if terms[k] is not None]
        mb[g] = len(rows)
        if rows:
            T[g] = br.run_sum(rows)
    m = int(mb.sum())
    row = {"label": int(label), "n_cells": len(cells), "n_profiles": m, "n_blocks": nb, "replicates": R, "n_failed": 0,
           "f_index0": -1, "lo_index": -1, "hi_index": -1, "status": 1, "index": np.full(R + 1, -1), "a": np.full(R + 1, np.nan),
           "near": np.zeros(R + 1, dtype=bool), "n_live": np.zeros(R + 1, dtype=np.int64), "hist": np.zeros(F, dtype=np.int64),
           "terms": T, "mb": mb, "picks": None}
    for f in ROW_FLOATS:
        row[f] = np.nan
    if nb < min_blocks or m < min_profiles:
        return row
    picks = picks_of(seed, label, R, nb)
    row["index"], row["a"], row["near"], row["n_live"] = replicates(T, mb, picks, mode, dtype)
    row["picks"] = picks
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
    ar = area_of(av, freqs[row["index"][1:][ok]].astype(dtype))
    lo, hi = int(x[klo]), int(x[khi])
    i0 = int(row["index"][0])
    row.update(f_index0=i0, lo_index=lo, hi_index=hi, status=(2 if lo == 0 else 0) + (4 if hi == F - 1 else 0),
               f0=float(freqs[i0]) if i0 >= 0 else np.nan, f_lo=float(freqs[lo]), f_hi=float(freqs[hi]),
               a0=row["a"][0], area0=area_of(row["a"][0], freqs[i0]) if i0 >= 0 else np.nan)
    for name, v in (("a", av), ("area", ar)):
        mean = seq_sum(v) / n_ok
        row[name + "_mean"] = mean
        row[name + "_sd"] = np.sqrt(seq_sum((v - mean) ** 2) / (n_ok - 1)) if n_ok > 1 else np.nan
        vs = np.sort(v)
        row[name + "_lo"], row[name + "_hi"] = vs[klo], vs[khi]
    return row


_ROWS = {}


def restate(case, mode, longdouble=False):
    """The restatement's rows of a case in label order."""
    key = (case["name"], mode, longdouble)
    if key not in _ROWS:
        terms = stage_of(case)
        nx = case["z"].shape[1]
        rows = []
        for l, pos in zip(*csr.group(case["labels"])):
            strike = br.strike_of(case["angle"][pos]) if case.get("seg_strike") is None else float(case["seg_strike"][int(l)])
            rows.append(bootstrap_reach([terms[k] for k in pos], case["cells"][pos], int(l), nx, case["de"], strike,
                                        case["frequencies"], mode, case["block_length"], case["R"], case["level"], case["seed"],
                                        case["min_profiles"], case["min_blocks"], np.longdouble if longdouble else np.float64))
        _ROWS[key] = rows
    return _ROWS[key]


# ---- comparing the device's tables with the restatement -----------------------------------------------------------------------
def compare(ref, table, hist, index, amp, freqs):
    """The device's rows, (S, F) histograms and (S, R + 1) indices and depth coefficients against ``ref``.  The integers match
    exactly, but for a replicate whose two best keys the restatement finds within NEAR: such replicates may be at most 0.1 % of
    all, and a reach that holds a flipped one is compared replicate by replicate only.  Floats - the two standard deviations
    like the others - are within RTOL of their own size.  Returns the figures: 'a' the largest relative difference of any
    float, 'sd' that of a_sd and area_sd alone."""
    out = {"reaches": len(ref), "booted": 0, "replicates": 0, "near": 0, "flipped": 0, "a": 0.0, "sd": 0.0}
    F = len(freqs)
    assert len(table) == len(ref)
    for s, (r, g) in enumerate(zip(ref, table)):
        L = r["label"]
        for f in ROW_INTS:
            assert int(g[f]) == r[f], (L, f, g[f], r[f])
        if r["status"] & 1:
            assert int(g["status"]) == r["status"], (L, g["status"], r["status"])
            for f in ("f_index0", "lo_index", "hi_index"):
                assert int(g[f]) == -1, (L, f)
            for f in ROW_FLOATS + DERIVED:
                assert np.isnan(g[f]), (L, f)
            assert (index[s][1:] == -1).all() and np.isnan(amp[s][1:]).all() and not hist[s].any(), L
            assert int(g["n_failed"]) == r["n_failed"], L
            continue
        assert int(g["status"]) & 1 == 0, (L, g["status"])
        out["booted"] += 1
        R = r["replicates"]
        out["replicates"] += R + 1
        out["near"] += int(r["near"].sum())
        diff = np.flatnonzero(index[s] != r["index"])
        assert r["near"][diff].all(), (L, "indices differ away from a near-tie", diff[:5], index[s][diff[:5]], r["index"][diff[:5]])
        out["flipped"] += len(diff)
        same = index[s] == r["index"]
        ok = same & (r["index"] >= 0)
        ra = r["a"].astype(np.float64)
        da = np.abs(amp[s][ok] - ra[ok]) / np.abs(ra[ok])
        assert np.isnan(amp[s][same & (r["index"] < 0)]).all(), L
        assert da.max(initial=0.0) <= RTOL, (L, "a", da.max())
        out["a"] = max(out["a"], float(da.max(initial=0.0)))
        assert np.array_equal(hist[s], np.bincount(index[s][1:][index[s][1:] >= 0], minlength=F)), L
        assert int(g["n_failed"]) == int((index[s][1:] < 0).sum()), L
        assert int(g["f_index0"]) == int(index[s][0]) and (np.isnan(g["a0"]) if index[s][0] < 0 else float(g["a0"]) == amp[s][0]), L
        if len(diff):
            continue
        assert int(g["n_failed"]) == r["n_failed"] and np.array_equal(hist[s], r["hist"]), L
        for f in ("f_index0", "lo_index", "hi_index", "status"):
            assert int(g[f]) == r[f], (L, f, g[f], r[f])
        for f in ("f0", "f_lo", "f_hi"):
            assert float(g[f]) == r[f] or (np.isnan(g[f]) and np.isnan(r[f])), (L, f)
        for f in ROW_FLOATS[3:]:
            want = float(r[f])
            if np.isnan(want):
                assert np.isnan(g[f]), (L, f)
                continue
            d = abs(float(g[f]) - want) / abs(want) if want != 0.0 else (0.0 if float(g[f]) == 0.0 else np.inf)
            assert d <= RTOL, (L, f, g[f], want)
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
                assert np.isclose(float(g[f]), want[w], rtol=1e-14, atol=0.0), (L, f)
            assert float(g["area0"]) == area_of(float(g["a0"]), float(g["f0"])), L
    assert out["near"] <= 1e-3 * max(1, out["replicates"]), out
    return out


# ---- the inputs of tests/test_gpu_channel_bootstrap.py ----------------------------------------------------------------------------
N, H, W = 160, 20, 1
NROWS70 = 103        # rows of the line that blocks of 1.5 cut into 70 blocks
FS8 = cr.freqs_of_sigma(np.geomspace(1.0, 8.0, 8))
F0 = float(cr.freqs_of_sigma([3.0])[0])
NAMES = ["nb 1 4 5 70", "R 1", "R 1000", "F 1", "F 64", "D 3", "a block of 130", "an empty block", "clipped by the edge",
         "a dead frequency", "no live frequency", "R 4096, F 64"]
_CASES = None


def line_cells(rows, off=0):
    """One cell per row of ``rows`` on the trough's line of synthetic_channel(N) (moved ``off`` columns)."""
    return np.clip(cr.line_cells(N, N, np.asarray(rows, dtype=np.int64)) + off, np.asarray(rows) * N, np.asarray(rows) * N + N - 1)


def spiked(rng, rows, holes):
    """A tilted plane with a little noise and, at the line's cell of every row in ``rows``, a trough one cell wide and 1 deep -
    the narrowest frequency the call takes, pi f de = 6, fits it - and the cells: (z, cells).  In the rows ``holes`` the
    points j = -3..3 of the profile at orientation 0 are NaN: there that frequency has no live pair."""
    z = 0.01 * np.arange(N)[None, :] + 0.02 * rng.standard_normal((N, N))
    cells = line_cells(rows)
    for r, c in zip(cells // N, cells % N):
        z[r, c] -= 1.0
        if r in holes:
            z[r, c - 3:c + 4] = np.nan
    return z, cells


def gpu_cases():
    """The cases as dicts: name, stage (the name under which stage one is kept), z, de, cells, labels, angle (one per cell),
    h, w, D, frequencies, block_length, R, level, seed, min_samples, min_profiles, min_blocks.  DEMs are 160 x 160, h = 20,
    w = 1 or 0, at most 300 cells.  Seeded: the same on every box."""
    global _CASES
    if _CASES is not None:
        return _CASES
    z = cr.channel_z(N, f0=F0, sigma=0.1)
    rng = np.random.default_rng(20261021)
    cases = []

    def add(name, stage, cells, labels, angle, zz=z, fs=FS8, bl=1.0, R=100, D=0, seed=7, mb=5, ms=4, w=W):
        cells = np.ascontiguousarray(cells, dtype=np.int64)
        angle = np.ascontiguousarray(np.broadcast_to(np.asarray(angle, dtype=np.float64), cells.shape))
        cases.append(dict(name=name, stage=stage, z=zz, de=1.0, cells=cells, labels=np.asarray(labels, dtype=np.int64), angle=angle,
                          h=H, w=w, D=D, frequencies=np.ascontiguousarray(fs, dtype=np.float64), block_length=float(bl), R=R,
                          level=0.95, seed=seed, min_samples=ms, min_profiles=1, min_blocks=mb))

    # one cell per row (t = 1.02 a row) and blocks of 1.5: reaches of 1, 4, 5 and 70 blocks, their cells interleaved
    cells = np.concatenate([np.repeat(line_cells([30]), 2) + [0, 1], line_cells(np.arange(34, 40), off=1),
                            line_cells(np.arange(44, 51), off=-1), line_cells(np.arange(25, 25 + NROWS70))])
    lab = np.repeat([6, 2, 9, 4], [2, 6, 7, NROWS70])
    perm = rng.permutation(len(cells))
    ang = 0.2 + 0.02 * rng.standard_normal(len(cells))
    base = (cells[perm], lab[perm], ang[perm])
    add(NAMES[0], "base", *base, bl=1.5, R=100)
    add(NAMES[1], "base", *base, bl=1.5, R=1)
    add(NAMES[2], "base", *base, bl=1.5, R=1000)
    add(NAMES[3], "F 1", *base, bl=1.5, fs=[F0])
    f64 = cr.freqs_of_sigma(np.geomspace(0.5, 20.0, 64))
    add(NAMES[4], "F 64", *base, bl=1.5, fs=f64)
    add(NAMES[5], "D 3", *base, bl=1.5, D=3)
    # 300 cells within a few columns of the line over 100 rows, blocks of 45: a block of more than 130 usable profiles
    rows = rng.integers(30, 130, 300)
    many = line_cells(rows, off=rng.integers(-2, 3, 300))
    add(NAMES[6], "many", many, np.ones(300, dtype=int), 0.2, bl=45.0, mb=2)
    # rows 66..93 are NaN: the cells of rows 76..83 have no usable profile, and blocks of 8 rows put them in a block alone
    zn = z.copy()
    zn[66:94, :] = np.nan
    hole = line_cells(np.arange(36, 124))
    add(NAMES[7], "hole", hole, np.full(len(hole), 3), 0.2, zz=zn, bl=8.0 / np.cos(0.2) - 1e-9)
    # the right edge clips the profiles: cells 3..24 columns from it
    edge = np.arange(40, 120) * N + (N - 3 - (np.arange(80) % 22))
    add(NAMES[8], "edge", edge, np.full(80, 5), 0.2, bl=4.0)
    # profiles along the rows (orientation 0, no swath), blocks of five rows; the holes sit in rows 50..54, the third block
    fd = np.concatenate([cr.freqs_of_sigma(np.geomspace(1.0, 8.0, 7)), [6.0 / np.pi]])
    zd, cd = spiked(rng, np.arange(40, 70), set(range(51, 55)))
    add(NAMES[9], "dead", cd, np.ones(30, dtype=int), 0.0, zz=zd, fs=fd, bl=5.0, R=200, w=0)
    # the one frequency pi f de = 6: reach 1 has a hole in every profile, reach 2 in none, reach 3 in its third block
    rows = np.concatenate([np.arange(20, 50), np.arange(60, 90), np.arange(100, 130)])
    zl, cl = spiked(rng, rows, set(range(20, 50)) | set(range(111, 115)))
    add(NAMES[10], "none live", cl, np.repeat([1, 2, 3], 30), 0.0, zz=zl, fs=[6.0 / np.pi], bl=5.0, R=200, w=0)
    # the top of the range: R = 4096 at F = 64
    add(NAMES[11], "F 64", *base, bl=1.5, fs=f64, R=4096)
    _CASES = cases
    return cases


# ---- the widening trough of docs/channels.md, "Intervals per reach" ---------------------------------------------------------------
WIDE = {"n": 600, "theta": 0.2, "h": 100, "w": 2, "D": 4, "noise": 0.3, "block_length": 30.0, "R": 1000, "seed": 7, "reach": 150.0}


def widening_z(span):
    """synthetic_channel(600, sigma=0.3) with the trough's width changing along the strike: sigma = 1.5 * 1.12^(14 + span c),
    c = clip(xrot / 150, -1, 1); the same noise draw, stored as float32."""
    n, theta = WIDE["n"], WIDE["theta"]
    x = np.linspace(-n / 2, n / 2, num=n, dtype=np.float64)
    th = np.pi / 2 - theta
    yrot = -x[None, :] * np.sin(th) + x[:, None] * np.cos(th)
    xrot = x[None, :] * np.cos(th) + x[:, None] * np.sin(th)
    c = np.clip(xrot / WIDE["reach"], -1.0, 1.0)
    f = 1.0 / (np.sqrt(2.0) * np.pi * 1.5 * 1.12 ** (14.0 + span * c))
    z = -np.exp(-(np.pi * f * yrot) ** 2) + 0.01 * yrot
    z += WIDE["noise"] * np.random.default_rng(20260101).standard_normal((n, n))
    return z.astype(np.float32).astype(np.float64)


def widening_case(span):
    """100 cells on the line - rows 150, 153, ..., 447, no offsets - as one reach, the 28 frequencies of the recovery."""
    n, theta = WIDE["n"], WIDE["theta"]
    cells = cr.line_cells(n, n, np.arange(150, 450, 3), theta)
    return dict(name="widening trough, span %g" % span, stage="widening %g" % span, z=widening_z(span), de=1.0,
                cells=np.ascontiguousarray(cells, dtype=np.int64), labels=np.ones(len(cells), dtype=np.int64),
                angle=np.full(len(cells), theta), h=WIDE["h"], w=WIDE["w"], D=WIDE["D"], frequencies=cr.REC["frequencies"],
                block_length=WIDE["block_length"], R=WIDE["R"], level=0.95, seed=WIDE["seed"], min_samples=4, min_profiles=1,
                min_blocks=5, delta=1.0)


# ... as the restatement measures it (tests/test_channel_bootstrap_host.py): per span and mode the interval of
# fit_channel_segments, the bootstrap's, and the replicates' histogram from its first to its last index that holds one
WIDE_SPANS = (0, 3)
# (fit_channel_segments: 13, [13, 13] in all four; the bootstrap: [13, 13] at span 0 and [12, 14] at span 3)
WIDE_HIST = {(0, "profile"): (13, [1000]), (0, "segment"): (13, [1000]),
             (3, "profile"): (11, [3, 216, 654, 126, 1]), (3, "segment"): (11, [1, 143, 680, 174, 2])}
