"""numpy restatement of sc_fit_segments (docs/segments.md, include/scarplet_hip.h), algebraically independent of the
device's route: per segment and age ONE ``np.linalg.lstsq`` on the full design matrix - a dummy intercept column and a
dummy slope column per usable profile plus the shared erf column, 2 n_profiles + 1 columns - never the per-profile
orthogonalisation the device uses.  The profiles are ``profile_reference.sample_profile``'s, the choice of the age is
``profile_reference.choose``'s.  The columns are scaled to unit norm before the solve (which changes the solution in no
way and makes the singular values lstsq returns those of the column-scaled matrix): their ratio is the condition
number the GPU tolerances are tied to."""
import numpy as np
from scipy.special import erf

import profile_reference as pr

ROW_FLOATS = ("kt", "kt_lo", "kt_hi", "a", "sse", "rmse")
ROW_INTS = ("n_cells", "n_profiles", "n", "dof")


def design(svals, kt):
    """The full design matrix of one age for the usable profiles' abscissae ``svals`` (a list of 1-D arrays)."""
    n = sum(len(s) for s in svals)
    X = np.zeros((n, 2 * len(svals) + 1))
    o = 0
    for c, s in enumerate(svals):
        X[o:o + len(s), 2 * c] = 1.0
        X[o:o + len(s), 2 * c + 1] = s
        X[o:o + len(s), -1] = erf(s / (2 * np.sqrt(kt)))
        o += len(s)
    return X


def fit_age(svals, pvals, kt):
    """(coefficients (c0_0, b_0, c0_1, b_1, ..., a), sse, per-profile sse, condition number) of one age."""
    X = design(svals, kt)
    p = np.concatenate(pvals)
    norm = np.linalg.norm(X, axis=0)
    coef, _, rank, sv = np.linalg.lstsq(X / norm, p, rcond=None)
    assert rank == X.shape[1], (rank, X.shape)
    coef = coef / norm
    res = p - X @ coef
    ends = np.cumsum([len(s) for s in svals])
    per = np.array([np.sum(r * r) for r in np.split(res, ends[:-1])])
    return coef, float(np.sum(res * res)), per, float(sv[0] / sv[-1])


def fit_segment(z, de, cells, sa, ca, h, w, ages, delta=1.0, min_samples=4, min_profiles=1):
    """One segment's row as a dict, plus 'curve' (sse per age), 'coefs' (A x (2 n_profiles + 1)), 'per' (A x
    n_profiles: each usable profile's sse), 'cond' (the largest condition number), 'ptp' (the largest peak-to-peak
    range of a usable profile), 'used' and 'cell_n' (one per cell) and 'rank' (cell -> its place among the usable)."""
    ny, nx = z.shape
    j = np.arange(-h, h + 1)
    svals, pvals, used, cell_n = [], [], [], []
    for k, cell in enumerate(cells):
        r, c = divmod(int(cell), nx)
        p = pr.sample_profile(z, float(r), float(c), sa[k], ca[k], h, w)
        ok = ~np.isnan(p)
        cell_n.append(int(ok.sum()))
        u = int((ok & (j < 0)).sum()) >= min_samples and int((ok & (j > 0)).sum()) >= min_samples
        used.append(int(u))
        if u:
            svals.append((j.astype(np.float64) * de)[ok])
            pvals.append(p[ok])
    m = len(svals)
    n = int(sum(len(s) for s in svals))
    row = {"n_cells": len(cells), "n_profiles": m, "n": n, "dof": n - 2 * m - 1, "kt_index": -1, "lo_index": -1,
           "hi_index": -1, "status": 1, "curve": np.full(len(ages), np.nan), "cond": 0.0, "ptp": np.nan,
           "used": np.array(used, dtype=np.int64), "cell_n": np.array(cell_n, dtype=np.int64)}
    for f in ROW_FLOATS:
        row[f] = np.nan
    if m < min_profiles or row["dof"] < 1:
        return row
    fits = [fit_age(svals, pvals, kt) for kt in ages]
    sse = np.array([f[1] for f in fits])
    # profile_reference.choose divides delta by (n - 3): hand it dof + 3
    best, lo, hi, status = pr.choose(sse, row["dof"] + 3, delta)
    row.update(kt_index=best, lo_index=lo, hi_index=hi, status=status, kt=float(ages[best]), kt_lo=float(ages[lo]),
               kt_hi=float(ages[hi]), a=float(fits[best][0][-1]), sse=float(sse[best]),
               rmse=float(np.sqrt(sse[best] / row["dof"])), curve=sse, coefs=np.array([f[0] for f in fits]),
               per=np.array([f[2] for f in fits]), cond=max(f[3] for f in fits),
               ptp=max(float(p.max() - p.min()) for p in pvals))
    return row


def group(labels):
    """(distinct positive labels ascending, for each the input positions of its cells in input order)."""
    labels = np.asarray(labels)
    keep = np.flatnonzero(labels > 0)
    order = keep[np.argsort(labels[keep], kind="stable")]
    lab, start = np.unique(labels[order], return_index=True)
    return lab, np.split(order, start[1:]) if len(lab) else []


def fit_segments(z, de, cells, labels, angle, h, w, ages, delta=1.0, min_samples=4, min_profiles=1):
    """Rows (a list of dicts, one per distinct positive label in ascending order, each with 'label' and 'where': the
    input positions of its cells) for ``cells`` with one label and one orientation each; h and w in cells."""
    z = np.asarray(z, dtype=np.float64)
    ages = np.asarray(ages, dtype=np.float64)
    cells = np.asarray(cells)
    angle = np.broadcast_to(np.asarray(angle, dtype=np.float64), (len(cells),))
    sa, ca = np.sin(angle), np.cos(angle)
    lab, where = group(labels)
    rows = []
    for l, pos in zip(lab, where):
        row = fit_segment(z, de, cells[pos], sa[pos], ca[pos], h, w, ages, delta, min_samples, min_profiles)
        row["label"], row["where"] = int(l), pos
        rows.append(row)
    return rows


def compare(ref, table, cell_table, curve, h, de, delta):
    """The device's tables (rows in label order, the cell table in input order of the kept cells given their input
    positions in ref[...]['where'], the (S, A) curves) against ``ref`` (fit_segments rows).  ``cell_table`` must be
    indexed by input position.  Asserts what is exact or within RTOL; returns the figures."""
    out = {"segments": len(ref), "fitted": 0, "ties": 0, "sse": 0.0, "coef": 0.0, "cond": 0.0}
    assert len(table) == len(ref)
    for s, (r, g) in enumerate(zip(ref, table)):
        L = r["label"]
        assert int(g["label"]) == L
        for f in ROW_INTS:
            assert int(g[f]) == r[f], (L, f, g[f], r[f])
        ct = cell_table[r["where"]]
        assert np.array_equal(ct["used"], r["used"]) and np.array_equal(ct["n"], r["cell_n"]), L
        assert np.all(ct["label"] == L)
        assert (int(g["status"]) & 1) == (r["status"] & 1), (L, g["status"], r["status"])
        if r["status"] == 1:
            assert int(g["kt_index"]) == -1 and int(g["lo_index"]) == -1 and int(g["hi_index"]) == -1
            assert all(np.isnan(g[f]) for f in ROW_FLOATS) and np.isnan(g["height"]), L
            assert np.isnan(curve[s]).all()
            assert np.isnan(ct["b"]).all() and np.isnan(ct["c0"]).all() and np.isnan(ct["sse"]).all()
            continue
        out["fitted"] += 1
        assert r["cond"] <= pr.COND_MAX, ("the inputs leave the tolerance's ground", L, r["cond"])
        out["cond"] = max(out["cond"], r["cond"])
        cv, dof = r["curve"], r["dof"]
        gi, glo, ghi = int(g["kt_index"]), int(g["lo_index"]), int(g["hi_index"])
        tie = False
        if gi != r["kt_index"]:
            assert abs(cv[gi] - r["sse"]) <= pr.RTOL * r["sse"], (L, gi, r["kt_index"], cv[gi], r["sse"])
            tie = True
        thr = cv[gi] * (1.0 + delta / dof)
        for gv, rv, i in ((glo, r["lo_index"], max(glo, r["lo_index"]) - 1), (ghi, r["hi_index"], min(ghi, r["hi_index"]) + 1)):
            if gv != rv:
                assert abs(cv[i] - thr) <= pr.RTOL * thr, (L, gv, rv, cv[i], thr)
                tie = True
        if tie:
            out["ties"] += 1
        else:
            assert int(g["status"]) == r["status"], (L, g["status"], r["status"])
        ds = max(abs(float(g["sse"]) - cv[gi]) / cv[gi], float(np.max(np.abs(curve[s] - cv) / cv)))
        coef = r["coefs"][gi]
        u = r["used"] == 1
        assert np.isnan(ct["b"][~u]).all() and np.isnan(ct["c0"][~u]).all() and np.isnan(ct["sse"][~u]).all(), L
        dc = max(abs(float(g["a"]) - coef[-1]), float(np.max(np.abs(ct["c0"][u] - coef[0:-1:2]))),
                 float(np.max(np.abs(ct["b"][u] - coef[1:-1:2]))) * h * de) / r["ptp"]
        # each profile's share of the pooled sum, against the pooled sum
        ds = max(ds, float(np.max(np.abs(ct["sse"][u] - r["per"][gi]))) / cv[gi])
        assert ds <= pr.RTOL, (L, "sse", ds)
        assert dc <= pr.RTOL, (L, "coefficients", dc)
        out["sse"], out["coef"] = max(out["sse"], ds), max(out["coef"], dc)
    assert out["ties"] <= pr.TIE_SHARE * max(1, out["segments"]), out
    return out


# ---- the noisy surface of docs/segments.md ------------------------------------------------------------------------------
def noisy_case():
    """(z, cells, angle): synthetic_scarp(600, sigma=0.5, theta=0.2) and 100 cells on the scarp's line - rows 150,
    153, ... 447, at the column where |yrot| is smallest."""
    n, theta = 600, 0.2
    z = pr.synthetic_z(n, sigma=0.5, theta=theta)
    x = np.linspace(-n / 2, n / 2, num=n)
    rows = np.arange(150, 450, 3)
    yrot = -x[None, :] * np.cos(theta) + x[rows][:, None] * np.sin(theta)
    cols = np.argmin(np.abs(yrot), axis=1)
    return z, rows.astype(np.int64) * n + cols, theta


# ---- the inputs of tests/test_gpu_segments.py -----------------------------------------------------------------------------
def gpu_cases():
    """The cases that need no search, as dicts: name, z, de, cells (int64), labels (one per cell, in shuffled order
    unless the name says otherwise), angle (one per cell), h, w (cells), ages, delta, min_samples, min_profiles.
    Seeded: the same on every box."""
    from scarplet_amd import _plan
    ages = _plan.age_grid()
    cases = []

    def add(name, z, de, cells, labels, angle, h, w, kt=ages, delta=1.0, ms=4, mp=1):
        cells = np.ascontiguousarray(cells, dtype=np.int64)
        angle = np.ascontiguousarray(np.broadcast_to(np.asarray(angle, dtype=np.float64), cells.shape))
        cases.append(dict(name=name, z=z, de=float(de), cells=cells, labels=np.asarray(labels, dtype=np.int64), angle=angle,
                          h=h, w=w, ages=np.asarray(kt, dtype=np.float64), delta=delta, min_samples=ms, min_profiles=mp))

    rng = np.random.default_rng(20261016)
    z = pr.synthetic_z(600)
    on = pr.scarp_cells(600, 120, rng, spread=3.0)
    ang = 0.2 + 0.05 * rng.standard_normal(120)
    lab = rng.integers(1, 9, 120) * 3                                     # eight segments, their cells interleaved
    # (the ages stop where the erf of the oldest is still bent over the profile: see docs/profiles.md, Limits)
    for h, w, na in ((100, 0, 35), (100, 5, 35), (30, 5, 35), (15, 2, 35)):
        add("synthetic h%d w%d" % (h, w), z, 1.0, on, lab, ang, h, w, kt=ages[:na], ms=min(h, 15))
    # segments of 1, 2, 64, 65 and 2100 cells in one call: both sides of the 64-profile block of the segmented sum,
    # and many blocks.  Short profiles and two young ages: the restatement's matrix has 4201 columns
    sizes = [1, 2, 64, 65, 2100]
    lab = np.repeat([5, 1, 9, 2, 7], sizes)
    big = pr.scarp_cells(600, len(lab), rng, spread=1.0)
    add("sizes 1 2 64 65 2100", z, 1.0, big, lab, 0.2 + 0.02 * rng.standard_normal(len(lab)), 5, 1, kt=[1.0, 3.0], ms=3)
    perm = rng.permutation(len(lab))[:400]                                # the same cells, fewer, in shuffled order
    add("shuffled order", z, 1.0, big[perm], lab[perm], 0.2, 30, 2, kt=ages[:24:2], ms=10, delta=4.0)
    add("repeated cells", z, 1.0, np.concatenate([np.repeat(on[:7], 3), on[:7]]), np.repeat([2, 1], [21, 7]), 0.2, 100, 5,
        ms=15, delta=0.0)
    add("one age", z, 1.0, on[:60], np.arange(60) % 3 + 1, 0.2, 100, 2, kt=[10.0], ms=15)
    add("64 ages", z, 1.0, on[:60], np.arange(60) % 3 + 1, 0.2, 100, 2, kt=10 ** np.linspace(0, 3.4, 64), ms=15)
    add("min_profiles 25", z, 1.0, on[:60], np.arange(60) % 3 + 1 + (np.arange(60) > 40), 0.2, 100, 2, ms=15, mp=25)
    add("no cell", z, 1.0, on[:0], on[:0], 0.2, 100, 5, ms=15)
    add("labels <= 0 only", z, 1.0, on[:5], [0, -1, 0, 0, -7], 0.2, 100, 5, ms=15)
    n = 300
    zb = pr.synthetic_z(n, seed=7)
    edge = np.concatenate([rng.integers(0, n, 40), rng.integers(0, n, 40) * n, rng.integers(0, n, 40) * n + n - 1,
                           (n - 1) * n + rng.integers(0, n, 40), rng.integers(0, 40, 60) * n + rng.integers(0, n, 60),
                           rng.integers(0, n, 60) * n + rng.integers(n - 40, n, 60)])
    add("borders", zb, 1.0, edge, rng.integers(1, 15, len(edge)), rng.uniform(-np.pi, np.pi, len(edge)), 100, 5, ms=20)
    # the corners at orientation 0 have nothing on one side: a segment none of whose cells is usable, next to one that is
    corners = np.array([0, n - 1, n * (n - 1), n * n - 1, 150 * n + 150, 151 * n + 150])
    add("unusable segment", zb, 1.0, corners, [4, 4, 4, 4, 6, 6], 0.0, 100, 5, ms=20)
    zn = pr.synthetic_z(400, seed=11).copy()
    zn[rng.random(zn.shape) < 0.004] = np.nan
    zn[180:200, 150:230] = np.nan
    add("NaN cells", zn, 1.0, rng.integers(0, zn.size, 250), rng.integers(1, 13, 250), rng.uniform(-np.pi / 2, np.pi / 2, 250),
        40, 3, ms=20)
    return cases


def restate(case):
    return fit_segments(case["z"], case["de"], case["cells"], case["labels"], case["angle"], case["h"], case["w"],
                        case["ages"], case["delta"], case["min_samples"], case["min_profiles"])
