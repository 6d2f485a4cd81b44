"""numpy restatement of sc_bootstrap_segments (docs/bootstrap.md, include/scarplet_hip.h), written from the definition:
the blocks along the strike, the per-profile terms See_ci and Sep_ci by projection (a QR of the columns 1 and s, never
the device's three passes), the integer draws in uint64 arithmetic, the replicates' argmax of Q_i = SSep_i^2 / SSee_i
and the rank rule of the percentiles.  The profiles are ``profile_reference.sample_profile``'s (through
``shift_reference.profile_of``), the grouping by label ``segment_reference.group``'s."""
import math

import numpy as np

import segment_reference as sr
import shift_reference as sh

NEAR = 1e-12         # a replicate whose two largest Q_i lie within this, relatively, may go either way
RTOL = 1e-9          # amplitudes against the device: the project's tolerance for fits against lstsq

U = np.uint64


def mix(z):
    """The splitmix64 finaliser on uint64 arrays (numpy's unsigned arithmetic wraps modulo 2^64)."""
    z = np.asarray(z, dtype=U)
    z = z ^ (z >> U(30))
    z = z * U(0xBF58476D1CE4E5B9)
    z = z ^ (z >> U(27))
    z = z * U(0x94D049BB133111EB)
    return z ^ (z >> U(31))


def draws(seed, label, R, nb):
    """(R, nb) int64: the block of draw k of replicate r = 1..R, for a segment of nb blocks and this label."""
    key = mix(np.array([seed], dtype=U) ^ (np.array([label], dtype=U) * U(0x9E3779B97F4A7C15)))
    r = np.arange(1, R + 1, dtype=U)[:, None]
    k = np.arange(nb, dtype=U)[None, :]
    u = mix(key + ((r << U(32)) | k))
    return (((u >> U(32)) * U(nb)) >> U(32)).astype(np.int64)


def strike_of(angles):
    """The axial mean of a segment's angles, the sums taken in sequence over the cells as given."""
    a = np.asarray(angles, dtype=np.float64)
    return 0.5 * math.atan2(np.cumsum(np.sin(2.0 * a))[-1], np.cumsum(np.cos(2.0 * a))[-1])


def blocks(cells, nx, de, strike, block_length):
    """The blocks of one segment: a list of arrays of positions into ``cells`` (in the order given), one per block that
    holds a cell, ascending along the strike."""
    cells = np.asarray(cells, dtype=np.int64)
    t = de * ((cells // nx).astype(np.float64) * np.cos(strike) + (cells % nx).astype(np.float64) * np.sin(strike))
    b = np.floor((t - t.min()) / block_length).astype(np.int64)
    return [np.flatnonzero(b == v) for v in np.unique(b)]


def profile_terms(z, de, cell, sa, ca, h, w, D, ages, min_samples):
    """(usable, See (A), Sep (A), Spp) of one cell: e and p with the span of (1, s) projected out, the erf column moved
    by the shift d of -D..D with the smallest sse at each age (tried in the order 0, -1, +1, ...)."""
    p, j, n, usable = sh.profile_of(z, cell, sa, ca, h, w, min_samples)
    A = len(ages)
    if not usable:
        return False, np.zeros(A), np.zeros(A), 0.0
    s = j.astype(np.float64) * de
    Q = np.linalg.qr(np.stack([np.ones_like(s), s], axis=1))[0]
    p2 = p - Q @ (Q.T @ p)
    order = sh.shift_order(D)
    E = np.stack([np.stack([sh.erf_column(j, d, de, kt) for d in order], axis=1) for kt in ages], axis=1)     # (n, A, ND)
    E2 = E - np.einsum("nk,kad->nad", Q, np.einsum("nk,nad->kad", Q, E))
    See = np.einsum("nad,nad->ad", E2, E2)
    Sep = np.einsum("nad,n->ad", E2, p2)
    res = p2[:, None, None] - (Sep / See)[None] * E2
    pick = np.argmin(np.einsum("nad,nad->ad", res, res), axis=1)          # (the first smallest in the order tried)
    i = np.arange(A)
    return True, See[i, pick], Sep[i, pick], float(p2 @ p2)


def run_sum(terms):
    """Rows summed as the device sums them: runs of 64 in sequence from the first, then the run sums in sequence."""
    tot = None
    for r0 in range(0, len(terms), 64):
        run = terms[r0]
        for v in terms[r0 + 1:r0 + 64]:
            run = run + v
        tot = run if tot is None else tot + run
    return tot


def ranks(n_ok, level):
    q = (1.0 - level) / 2.0
    return int(math.floor(q * n_ok)), int(math.ceil((1.0 - q) * n_ok)) - 1


def replicate(T, pick):
    """(index or -1, a, near) of the replicate that takes the rows ``pick`` of the block terms T (nb, A, 2)."""
    S = T[pick, :, 0].sum(axis=0)
    P = T[pick, :, 1].sum(axis=0)
    if not np.all((S > 0) & np.isfinite(S)):
        return -1, np.nan, False
    with np.errstate(invalid="ignore", over="ignore"):
        Qv = P * P / S
    Qv = np.where(np.isnan(Qv), -np.inf, Qv)
    best = int(np.argmax(Qv))
    if Qv[best] == -np.inf:
        return -1, np.nan, False
    two = np.sort(Qv)[-2:]
    near = len(Qv) > 1 and (two[1] - two[0]) <= NEAR * abs(two[1])
    return best, float(P[best] / S[best]), bool(near)


def bootstrap_segment(z, de, cells, sa, ca, label, nx, strike, h, w, D, ages, block_length, R, level, seed, min_samples,
                      min_profiles, min_blocks):
    """One segment's row as a dict: the fields of sc_segment_boot, plus 'index' and 'a' (R + 1, replicate 0 first),
    'near' (R + 1 bools), 'hist' (A) and 'terms' (nb, A, 2)."""
    A = len(ages)
    blk = blocks(cells, nx, de, strike, block_length)
    nb = len(blk)
    T = np.zeros((nb, A, 2))
    m = 0
    for g, pos in enumerate(blk):
        rows = []
        for k in pos:
            ok, See, Sep, _ = profile_terms(z, de, cells[k], sa[k], ca[k], h, w, D, ages, min_samples)
            if ok:
                rows.append(np.stack([See, Sep], axis=1))
        m += len(rows)
        if rows:
            T[g] = run_sum(rows)
    row = {"label": int(label), "n_cells": len(cells), "n_profiles": m, "n_blocks": nb, "replicates": R, "n_failed": 0,
           "kt_index0": -1, "lo_index": -1, "hi_index": -1, "status": 1, "index": np.full(R + 1, -1), "a": np.full(R + 1, np.nan),
           "near": np.zeros(R + 1, dtype=bool), "hist": np.zeros(A, dtype=np.int64), "terms": T}
    for f in ("kt0", "kt_lo", "kt_hi", "a0", "a_mean", "a_sd", "a_lo", "a_hi"):
        row[f] = np.nan
    if nb < min_blocks or m < min_profiles:
        return row
    picks = np.concatenate([np.arange(nb)[None, :], draws(seed, label, R, nb)])
    for r in range(R + 1):
        row["index"][r], row["a"][r], row["near"][r] = replicate(T, picks[r])
    ok = row["index"][1:] >= 0
    n_ok = int(ok.sum())
    row["n_failed"] = R - n_ok
    row["hist"] = np.bincount(row["index"][1:][ok], minlength=A)
    if n_ok == 0:
        return row
    klo, khi = ranks(n_ok, level)
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


def bootstrap_segments(z, de, cells, labels, angle, h, w, ages, block_length, R, level=0.95, seed=0, D=0, min_samples=4,
                       min_profiles=1, min_blocks=5, seg_strike=None):
    """Rows (a list of dicts, one per distinct positive label in ascending order) for ``cells`` with one label and one
    orientation each; h, w and D in cells.  ``seg_strike``: {label: strike} instead of the cells' axial mean."""
    z = np.asarray(z, dtype=np.float64)
    ages = np.asarray(ages, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.int64)
    angle = np.broadcast_to(np.asarray(angle, dtype=np.float64), (len(cells),))
    sa, ca = np.sin(angle), np.cos(angle)
    lab, where = sr.group(labels)
    rows = []
    for l, pos in zip(lab, where):
        strike = strike_of(angle[pos]) if seg_strike is None else float(seg_strike[int(l)])
        rows.append(bootstrap_segment(z, de, cells[pos], sa[pos], ca[pos], int(l), z.shape[1], strike, h, w, D, ages,
                                      float(block_length), R, level, seed, min_samples, min_profiles, min_blocks))
    return rows


def compare(ref, table, hist, index, amp):
    """The device's rows, (S, A) histograms and (S, R + 1) indices and amplitudes against ``ref``.  The integers match
    exactly, but for a replicate whose two largest Q_i the restatement finds within NEAR: such replicates may be at
    most 0.1 % of all, and a segment that holds one is compared replicate by replicate only.  Returns the figures."""
    out = {"segments": len(ref), "booted": 0, "replicates": 0, "near": 0, "flipped": 0, "a": 0.0}
    assert len(table) == len(ref)
    for s, (r, g) in enumerate(zip(ref, table)):
        L = r["label"]
        for f in ("label", "n_cells", "n_profiles", "n_blocks", "replicates"):
            assert int(g[f]) == r[f], (L, f, g[f], r[f])
        assert (int(g["status"]) == 1) == (r["status"] == 1), (L, g["status"], r["status"])
        if r["status"] == 1:
            for f in ("kt_index0", "lo_index", "hi_index"):
                assert int(g[f]) == -1, (L, f)
            for f in ("kt0", "kt_lo", "kt_hi", "a0", "a_mean", "a_sd", "a_lo", "a_hi", "height0", "height_lo", "height_hi"):
                assert np.isnan(g[f]), (L, f)
            assert (index[s][1:] == -1).all() and np.isnan(amp[s][1:]).all() and not hist[s].any(), L
            continue
        out["booted"] += 1
        R = r["replicates"]
        out["replicates"] += R + 1
        out["near"] += int(r["near"].sum())
        diff = np.flatnonzero(index[s] != r["index"])
        assert r["near"][diff].all(), (L, "indices differ away from a near-tie", diff[:5], index[s][diff[:5]], r["index"][diff[:5]])
        out["flipped"] += len(diff)
        same = index[s] == r["index"]
        ok = same & (r["index"] >= 0)
        da = np.abs(amp[s][ok] - r["a"][ok]) / np.abs(r["a"][ok])
        assert np.isnan(amp[s][same & (r["index"] < 0)]).all(), L
        assert da.max(initial=0.0) <= RTOL, (L, "a", da.max())
        out["a"] = max(out["a"], float(da.max(initial=0.0)))
        assert np.array_equal(hist[s], np.bincount(index[s][1:][index[s][1:] >= 0], minlength=hist.shape[1])), L
        assert int(g["n_failed"]) == int((index[s][1:] < 0).sum()), L
        if len(diff):
            continue
        assert int(g["n_failed"]) == r["n_failed"] and np.array_equal(hist[s], r["hist"]), L
        for f in ("kt_index0", "lo_index", "hi_index", "status"):
            assert int(g[f]) == r[f], (L, f, g[f], r[f])
        for f in ("kt0", "kt_lo", "kt_hi"):
            assert float(g[f]) == r[f], (L, f)
        for f in ("a0", "a_mean", "a_sd", "a_lo", "a_hi"):
            if np.isnan(r[f]):
                assert np.isnan(g[f]), (L, f)
                continue
            d = abs(float(g[f]) - r[f]) / abs(r[f])
            assert d <= RTOL, (L, f, g[f], r[f])
            out["a"] = max(out["a"], d)
        assert float(g["height0"]) == 2.0 * float(g["a0"]) and float(g["height_lo"]) == 2.0 * float(g["a_lo"])
        assert float(g["height_hi"]) == 2.0 * float(g["a_hi"])
    assert out["near"] <= 1e-3 * max(1, out["replicates"]), out
    return out


# ---- the inputs of tests/test_gpu_bootstrap.py ------------------------------------------------------------------------------
N, H, W = 160, 20, 1
NROWS70 = 103         # rows of the line that blocks of 1.5 cut into 70 blocks


def line_cells(rows, theta=0.2, off=0):
    """One cell per row of ``rows`` on the scarp's line of synthetic_scarp(N, theta) (moved ``off`` columns)."""
    x = np.linspace(-N / 2, N / 2, num=N)
    rows = np.asarray(rows, dtype=np.int64)
    yrot = -x[None, :] * np.cos(theta) + x[rows][:, None] * np.sin(theta)
    return rows * N + np.clip(np.argmin(np.abs(yrot), axis=1) + off, 0, N - 1)


def gpu_cases():
    """The cases as dicts: name, z, cells, labels, angle (one per cell), ages, block_length, R, D, seed, min_blocks,
    min_samples - all at de = 1, h = 20, w = 1 on a 160 x 160 synthetic_scarp with noise.  Seeded: the same on every box."""
    import profile_reference as pr
    from scarplet_amd import _plan
    ages = _plan.age_grid()
    z = pr.synthetic_z(N, sigma=0.3)
    rng = np.random.default_rng(20261020)
    cases = []

    def add(name, cells, labels, angle, zz=z, kt=ages, bl=1.0, R=100, D=0, seed=7, mb=5, ms=4):
        cells = np.ascontiguousarray(cells, dtype=np.int64)
        angle = np.ascontiguousarray(np.broadcast_to(np.asarray(angle, dtype=np.float64), cells.shape))
        cases.append(dict(name=name, z=zz, cells=cells, labels=np.asarray(labels, dtype=np.int64), angle=angle,
                          ages=np.asarray(kt, dtype=np.float64), block_length=float(bl), R=R, D=D, seed=seed, min_blocks=mb,
                          min_samples=ms))

    # one cell per row (t = 1.02 a row) and blocks of 1.5: segments of 1, 4, 5 and 70 blocks, their cells interleaved
    cells = np.concatenate([np.repeat(line_cells([30]), 2) + [0, 1], line_cells(np.arange(34, 40), off=1),
                            line_cells(np.arange(44, 51), off=-1), line_cells(np.arange(25, 25 + NROWS70))])
    lab = np.repeat([6, 2, 9, 4], [2, 6, 7, NROWS70])
    perm = rng.permutation(len(cells))
    ang = 0.2 + 0.02 * rng.standard_normal(len(cells))
    base = (cells[perm], lab[perm], ang[perm])
    add("nb 1 4 5 70", *base, bl=1.5, R=100)
    add("R 1", *base, bl=1.5, R=1)
    add("R 1000", *base, bl=1.5, R=1000)
    add("one age", *base, bl=1.5, kt=[10.0])
    add("64 ages", *base, bl=1.5, kt=10 ** np.linspace(0, 2.0, 64))
    add("D 3", *base, bl=1.5, D=3, R=100)
    # 300 cells within a few columns of the line over 100 rows, blocks of 45: a block of more than 130 usable profiles
    many = line_cells(rng.integers(30, 130, 300)) + rng.integers(-2, 3, 300)
    add("a block of 130", many, np.ones(300, dtype=int), 0.2, bl=45.0, mb=2)
    # rows 70..89 are NaN: the cells of rows 76..83 have no usable profile, and blocks of 8 rows put them in a block alone
    zn = z.copy()
    zn[66:94, :] = np.nan
    hole = line_cells(np.arange(36, 124))
    add("an empty block", hole, np.full(len(hole), 3), 0.2, zz=zn, bl=8.0 / np.cos(0.2) - 1e-9)
    # the right edge clips the profiles: cells 3..24 columns from it
    edge = np.arange(40, 120) * N + (N - 3 - (np.arange(80) % 22))
    add("clipped by the edge", edge, np.full(80, 5), 0.2, bl=4.0, ms=4)
    return cases


def restate(case):
    return bootstrap_segments(case["z"], 1.0, case["cells"], case["labels"], case["angle"], H, W, case["ages"],
                              case["block_length"], case["R"], 0.95, case["seed"], case["D"], case["min_samples"], 1,
                              case["min_blocks"])
