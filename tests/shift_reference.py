"""numpy restatement of the centre shift of sc_fit_profiles_shift / sc_fit_segments_shift (docs/profiles.md, "The centre
shift"; docs/segments.md), algebraically independent of the device's route: for a single profile ``np.linalg.lstsq`` on
the three columns ``1, s, erf((j - d) de / (2 sqrt(kt)))`` for EACH (cell, age, shift); for a segment ONE lstsq per age on
the full design matrix, each profile's erf column shifted by a given ``d_ci``.  The profiles are
``profile_reference.sample_profile``'s, the walk of the interval ``profile_reference.choose``'s."""
import numpy as np
from scipy.special import erf

import profile_reference as pr
import segment_reference as sr

RTOL, COND_MAX, TIE_SHARE = pr.RTOL, pr.COND_MAX, pr.TIE_SHARE


def shift_order(D):
    """The candidates in the order they are tried: 0, -1, +1, -2, +2, ..."""
    return [0] + [v for k in range(1, D + 1) for v in (-k, k)]


def erf_column(j, d, de, kt):
    """Row j - d of the table: the erf of the point j when the step sits d cells along the profile."""
    return erf((j - d).astype(np.float64) * de / (2 * np.sqrt(kt)))


def fit_pair(j, p, de, kt, d):
    """((c0, b, a), sse) of one (age, shift): float64 lstsq on three columns; j the valid points' indices."""
    s = j.astype(np.float64) * de
    X = np.stack([np.ones_like(s), s, erf_column(j, d, de, kt)], axis=1)
    coef = np.linalg.lstsq(X, p, rcond=None)[0]
    res = p - (coef[0] + coef[1] * s + coef[2] * X[:, 2])
    return coef, float(np.sum(res * res))


def conds(j, de, ages, order):
    """Condition numbers of the column-scaled design matrices of every (age, shift): (A, ND)."""
    s = j.astype(np.float64) * de
    X = np.empty((len(ages), len(order), len(j), 3))
    X[..., 0] = 1.0
    X[..., 1] = s
    for i, kt in enumerate(ages):
        for q, d in enumerate(order):
            X[i, q, :, 2] = erf_column(j, d, de, kt)
    X = X / np.linalg.norm(X, axis=2, keepdims=True)
    sv = np.linalg.svd(X, compute_uv=False)
    return sv[..., 0] / sv[..., -1]


def profile_of(z, cell, sa, ca, h, w, min_samples):
    """(p, valid j, n, usable) of one cell."""
    nx = z.shape[1]
    r, c = divmod(int(cell), nx)
    p = pr.sample_profile(z, float(r), float(c), sa, ca, h, w)
    j = np.arange(-h, h + 1)
    ok = ~np.isnan(p)
    usable = int((ok & (j < 0)).sum()) >= min_samples and int((ok & (j > 0)).sum()) >= min_samples
    return p[ok], j[ok], int(ok.sum()), usable


def fit_cell(z, de, cell, sa, ca, h, w, D, ages, delta=1.0, min_samples=4):
    """One cell's row as a dict: the fields of sc_profile_shift_fit, plus 'dof', 'grid' (A x ND: sse of every (age,
    candidate) in the order of shift_order), 'coefs' (A x ND x 3: c0, b, a), 'curve' (sse*), 'shifts' (d_i), 'cond' (the
    largest condition number), 'ptp' and 'usable' (the min_samples rule alone, which is what a segment asks)."""
    order = shift_order(D)
    A = len(ages)
    p, j, n, usable = profile_of(z, cell, sa, ca, h, w, min_samples)
    dof = n - 3 - (1 if D > 0 else 0)
    row = {"cell": int(cell), "n": n, "dof": dof, "kt_index": -1, "lo_index": -1, "hi_index": -1, "status": 1,
           "shift_index": 0, "shift": np.nan, "curve": np.full(A, np.nan), "shifts": np.zeros(A, dtype=np.int64),
           "cond": 0.0, "ptp": np.nan, "usable": usable, "order": order}
    for f in pr.ROW_FLOATS:
        row[f] = np.nan
    if not usable:
        return row
    grid = np.empty((A, len(order)))
    coefs = np.empty((A, len(order), 3))
    for i, kt in enumerate(ages):
        for q, d in enumerate(order):
            coefs[i, q], grid[i, q] = fit_pair(j, p, de, kt, d)
    pick = np.argmin(grid, axis=1)                                         # the first smallest in the order tried
    row.update(grid=grid, coefs=coefs, shifts=np.array(order)[pick], curve=grid[np.arange(A), pick],
               cond=float(conds(j, de, ages, order).max()), ptp=float(p.max() - p.min()))
    if dof < 1:
        row["curve"] = np.full(A, np.nan)
        row["shifts"] = np.zeros(A, dtype=np.int64)
        return row
    best, lo, hi, status = pr.choose(row["curve"], dof + 3, delta)         # (choose divides delta by n - 3)
    d = int(row["shifts"][best])
    c0, b, a = (float(v) for v in coefs[best, pick[best]])
    sse = float(row["curve"][best])
    row.update(kt_index=best, lo_index=lo, hi_index=hi, status=status + (8 if D > 0 and abs(d) == D else 0),
               shift_index=d, shift=d * de, kt=float(ages[best]), kt_lo=float(ages[lo]), kt_hi=float(ages[hi]), a=a, b=b,
               c0=c0, sse=sse, rmse=float(np.sqrt(sse / dof)))
    return row


def fit_profiles(z, de, cells, angle, h, w, D, ages, delta=1.0, min_samples=4):
    z = np.asarray(z, dtype=np.float64)
    ages = np.asarray(ages, dtype=np.float64)
    angle = np.broadcast_to(np.asarray(angle, dtype=np.float64), (len(cells),))
    sa, ca = np.sin(angle), np.cos(angle)
    return [fit_cell(z, de, cells[k], sa[k], ca[k], h, w, D, ages, delta, min_samples) for k in range(len(cells))]


def check_shifts(r, shifts, curve=None):
    """One cell's device shifts d_i (and sse* curve) against its restatement row: a d_i that differs must have been
    decided within RTOL.  Returns the number of ages so decided."""
    ties = 0
    pos = {d: q for q, d in enumerate(r["order"])}
    for i, d in enumerate(shifts):
        d = int(d)
        assert d in pos, (r["cell"], i, d)
        if d != r["shifts"][i]:
            assert abs(r["grid"][i, pos[d]] - r["curve"][i]) <= RTOL * r["curve"][i], \
                (r["cell"], i, d, r["shifts"][i], r["grid"][i, pos[d]], r["curve"][i])
            ties += 1
    if curve is not None:
        assert float(np.max(np.abs(np.asarray(curve) - r["curve"]) / r["curve"])) <= RTOL, (r["cell"], "sse*")
    return ties


def compare_rows(ref, table, curve, shifts, h, de, D, delta):
    """The device's table, (K, A) sse* curves and (K, A) shifts against ``ref`` (fit_cell rows).  Asserts what is exact
    or within RTOL; returns the figures.  A cell counts as a tie when an index or a shift of it differs from the
    restatement's and was decided within RTOL."""
    out = {"cells": len(ref), "fitted": 0, "ties": 0, "sse": 0.0, "coef": 0.0, "cond": 0.0}
    for k, r in enumerate(ref):
        g = table[k]
        assert int(g["n"]) == r["n"], (r["cell"], g["n"], r["n"])
        assert (int(g["status"]) & 1) == (r["status"] & 1), (r["cell"], g["status"], r["status"])
        if r["status"] == 1:
            assert int(g["kt_index"]) == -1 and int(g["lo_index"]) == -1 and int(g["hi_index"]) == -1, r["cell"]
            assert all(np.isnan(g[f]) for f in pr.ROW_FLOATS) and np.isnan(g["shift"]) and int(g["shift_index"]) == 0
            assert np.isnan(curve[k]).all() and not shifts[k].any()
            continue
        out["fitted"] += 1
        assert r["cond"] <= COND_MAX, ("the inputs leave the tolerance's ground", r["cell"], r["cond"])
        out["cond"] = max(out["cond"], r["cond"])
        tie = check_shifts(r, shifts[k], curve[k]) > 0
        cv, dof = r["curve"], r["dof"]
        gi, glo, ghi = int(g["kt_index"]), int(g["lo_index"]), int(g["hi_index"])
        if gi != r["kt_index"]:
            assert abs(cv[gi] - r["sse"]) <= RTOL * r["sse"], (r["cell"], gi, r["kt_index"], cv[gi], r["sse"])
            tie = True
        thr = cv[gi] * (1.0 + delta / dof)
        for gv, rv, i in ((glo, r["lo_index"], max(glo, r["lo_index"]) - 1), (ghi, r["hi_index"], min(ghi, r["hi_index"]) + 1)):
            if gv != rv:
                assert abs(cv[i] - thr) <= RTOL * thr, (r["cell"], gv, rv, cv[i], thr)
                tie = True
        d = int(g["shift_index"])
        assert d == int(shifts[k][gi]) and float(g["shift"]) == d * de, (r["cell"], d, shifts[k][gi])
        assert int(g["status"]) == (2 if glo == 0 else 0) + (4 if ghi == len(cv) - 1 else 0) + (8 if D > 0 and abs(d) == D else 0)
        if tie:
            out["ties"] += 1
        else:
            assert int(g["status"]) == r["status"] and d == r["shift_index"], (r["cell"], g["status"], r["status"])
        q = r["order"].index(d)
        ds = max(abs(float(g["sse"]) - r["grid"][gi, q]) / r["grid"][gi, q], abs(float(g["sse"]) - curve[k][gi]) / curve[k][gi])
        c0, b, a = r["coefs"][gi, q]
        dc = max(abs(float(g["c0"]) - c0), abs(float(g["b"]) - b) * h * de, abs(float(g["a"]) - a)) / r["ptp"]
        assert ds <= RTOL, (r["cell"], "sse", ds)
        assert dc <= RTOL, (r["cell"], "coefficients", dc)
        assert float(g["rmse"]) == float(np.sqrt(g["sse"] / dof)) and float(g["height"]) == 2.0 * float(g["a"])
        out["sse"], out["coef"] = max(out["sse"], ds), max(out["coef"], dc)
    assert out["ties"] <= TIE_SHARE * max(1, out["cells"]), out
    return out


# ---- segments -----------------------------------------------------------------------------------------------------------
def fit_segment(z, de, cells, sa, ca, h, w, D, ages, shifts, delta=1.0, min_samples=4, min_profiles=1):
    """segment_reference.fit_segment with profile c's erf column shifted by shifts[c, i] at age i (``shifts``: one row
    per cell of the segment, the rows of unusable cells ignored): one lstsq per age on the full design matrix."""
    jv, pv, used, cell_n = [], [], [], []
    for k, cell in enumerate(cells):
        p, j, n, usable = profile_of(z, cell, sa[k], ca[k], h, w, min_samples)
        cell_n.append(n)
        used.append(int(usable))
        if usable:
            jv.append(j)
            pv.append(p)
    m, n = len(jv), int(sum(len(j) for j in jv))
    dof = n - 2 * m - 1 - (m if D > 0 else 0)
    A = len(ages)
    row = {"n_cells": len(cells), "n_profiles": m, "n": n, "dof": dof, "kt_index": -1, "lo_index": -1, "hi_index": -1,
           "status": 1, "curve": np.full(A, np.nan), "cond": 0.0, "ptp": np.nan,
           "used": np.array(used, dtype=np.int64), "cell_n": np.array(cell_n, dtype=np.int64)}
    for f in sr.ROW_FLOATS:
        row[f] = np.nan
    if m < min_profiles or dof < 1:
        return row
    du = np.asarray(shifts)[row["used"] == 1]
    fits = []
    for i, kt in enumerate(ages):
        X = np.zeros((n, 2 * m + 1))
        o = 0
        for c, j in enumerate(jv):
            X[o:o + len(j), 2 * c] = 1.0
            X[o:o + len(j), 2 * c + 1] = j.astype(np.float64) * de
            X[o:o + len(j), -1] = erf_column(j, int(du[c, i]), de, kt)
            o += len(j)
        p = np.concatenate(pv)
        norm = np.linalg.norm(X, axis=0)
        coef, _, rank, sv = np.linalg.lstsq(X / norm, p, rcond=None)
        assert rank == X.shape[1], (rank, X.shape)
        coef = coef / norm
        res = p - X @ coef
        ends = np.cumsum([len(j) for j in jv])
        fits.append((coef, float(np.sum(res * res)), np.array([np.sum(v * v) for v in np.split(res, ends[:-1])]),
                     float(sv[0] / sv[-1])))
    sse = np.array([f[1] for f in fits])
    best, lo, hi, status = pr.choose(sse, dof + 3, delta)
    if D > 0 and np.any(np.abs(du[:, best]) == D):
        status += 8
    row.update(kt_index=best, lo_index=lo, hi_index=hi, status=status, kt=float(ages[best]), kt_lo=float(ages[lo]),
               kt_hi=float(ages[hi]), a=float(fits[best][0][-1]), sse=float(sse[best]), rmse=float(np.sqrt(sse[best] / dof)),
               curve=sse, coefs=np.array([f[0] for f in fits]), per=np.array([f[2] for f in fits]),
               cond=max(f[3] for f in fits), ptp=max(float(p.max() - p.min()) for p in pv), du=du)
    return row


def fit_segments(z, de, cells, labels, angle, h, w, D, ages, shifts, delta=1.0, min_samples=4, min_profiles=1):
    """Rows as segment_reference.fit_segments gives them; ``shifts`` (K, A) in input order."""
    z = np.asarray(z, dtype=np.float64)
    ages = np.asarray(ages, dtype=np.float64)
    cells = np.asarray(cells)
    angle = np.broadcast_to(np.asarray(angle, dtype=np.float64), (len(cells),))
    sa, ca = np.sin(angle), np.cos(angle)
    lab, where = sr.group(labels)
    rows = []
    for l, pos in zip(lab, where):
        row = fit_segment(z, de, cells[pos], sa[pos], ca[pos], h, w, D, ages, np.asarray(shifts)[pos], delta, min_samples,
                          min_profiles)
        row["label"], row["where"] = int(l), pos
        rows.append(row)
    return rows


def compare_segments(ref, table, cell_table, curve, h, de, D, delta):
    """segment_reference.compare for the shifted call: ``ref`` was computed WITH the device's shifts, so what is left
    to differ is the joint fit."""
    out = {"segments": len(ref), "fitted": 0, "ties": 0, "sse": 0.0, "coef": 0.0, "cond": 0.0}
    assert len(table) == len(ref)
    for s, (r, g) in enumerate(zip(ref, table)):
        L = r["label"]
        assert int(g["label"]) == L
        for f in sr.ROW_INTS:
            assert int(g[f]) == r[f], (L, f, g[f], r[f])
        ct = cell_table[r["where"]]
        assert np.array_equal(ct["used"], r["used"]) and np.array_equal(ct["n"], r["cell_n"]), L
        assert np.all(ct["label"] == L)
        assert (int(g["status"]) & 1) == (r["status"] & 1), (L, g["status"], r["status"])
        if r["status"] == 1:
            assert int(g["kt_index"]) == -1 and int(g["lo_index"]) == -1 and int(g["hi_index"]) == -1
            assert all(np.isnan(g[f]) for f in sr.ROW_FLOATS) and np.isnan(g["height"]), L
            assert np.isnan(curve[s]).all()
            assert np.isnan(ct["b"]).all() and np.isnan(ct["c0"]).all() and np.isnan(ct["sse"]).all()
            assert np.isnan(ct["shift"]).all() and not ct["shift_index"].any()
            continue
        out["fitted"] += 1
        assert r["cond"] <= COND_MAX, ("the inputs leave the tolerance's ground", L, r["cond"])
        out["cond"] = max(out["cond"], r["cond"])
        cv, dof = r["curve"], r["dof"]
        gi, glo, ghi = int(g["kt_index"]), int(g["lo_index"]), int(g["hi_index"])
        tie = False
        if gi != r["kt_index"]:
            assert abs(cv[gi] - r["sse"]) <= RTOL * r["sse"], (L, gi, r["kt_index"], cv[gi], r["sse"])
            tie = True
        thr = cv[gi] * (1.0 + delta / dof)
        for gv, rv, i in ((glo, r["lo_index"], max(glo, r["lo_index"]) - 1), (ghi, r["hi_index"], min(ghi, r["hi_index"]) + 1)):
            if gv != rv:
                assert abs(cv[i] - thr) <= RTOL * thr, (L, gv, rv, cv[i], thr)
                tie = True
        u = r["used"] == 1
        assert np.array_equal(ct["shift_index"][u], r["du"][:, gi]) and not ct["shift_index"][~u].any(), L
        assert np.array_equal(ct["shift"][u], r["du"][:, gi] * de) and np.isnan(ct["shift"][~u]).all(), L
        at_end = 8 if D > 0 and np.any(np.abs(r["du"][:, gi]) == D) else 0
        assert int(g["status"]) == (2 if glo == 0 else 0) + (4 if ghi == len(cv) - 1 else 0) + at_end, (L, g["status"])
        if tie:
            out["ties"] += 1
        else:
            assert int(g["status"]) == r["status"], (L, g["status"], r["status"])
        ds = max(abs(float(g["sse"]) - cv[gi]) / cv[gi], float(np.max(np.abs(curve[s] - cv) / cv)))
        coef = r["coefs"][gi]
        assert np.isnan(ct["b"][~u]).all() and np.isnan(ct["c0"][~u]).all() and np.isnan(ct["sse"][~u]).all(), L
        dc = max(abs(float(g["a"]) - coef[-1]), float(np.max(np.abs(ct["c0"][u] - coef[0:-1:2]))),
                 float(np.max(np.abs(ct["b"][u] - coef[1:-1:2]))) * h * de) / r["ptp"]
        ds = max(ds, float(np.max(np.abs(ct["sse"][u] - r["per"][gi]))) / cv[gi])
        assert ds <= RTOL, (L, "sse", ds)
        assert dc <= RTOL, (L, "coefficients", dc)
        assert float(g["rmse"]) == float(np.sqrt(g["sse"] / dof)) and float(g["height"]) == 2.0 * float(g["a"])
        out["sse"], out["coef"] = max(out["sse"], ds), max(out["coef"], dc)
    assert out["ties"] <= TIE_SHARE * max(1, out["segments"]), out
    return out


# ---- the offset case of docs/segments.md ------------------------------------------------------------------------------------
def offset_case(sigma=0.5, offsets=True):
    """(z, cells, angle, offsets): the surface and the 100 cells of segment_reference.noisy_case(), each cell moved along
    its row by a uniform integer offset in -6..6 (np.random.default_rng(3)); ``sigma=0`` for the noise-free surface."""
    z, cells, theta = sr.noisy_case()
    if sigma != 0.5:
        z = pr.synthetic_z(600, sigma=sigma, theta=theta)
    off = np.random.default_rng(3).integers(-6, 7, len(cells)) if offsets else np.zeros(len(cells), dtype=np.int64)
    return z, cells + off, theta, off


# ---- the inputs of tests/test_gpu_shift.py ----------------------------------------------------------------------------------
def profile_cases():
    """The single-profile cases as dicts: name, z, de, cells, angle, h, w, D, ages, delta, min_samples.  The age grids stop
    where the restatement's column-scaled condition number passes COND_MAX at some (age, shift): compare_rows asserts
    it.  Seeded: the same on every box."""
    from scarplet_amd import _plan
    ages = _plan.age_grid()
    cases = []

    def add(name, z, de, cells, angle, h, w, D, kt, delta=1.0, ms=4):
        cells = np.ascontiguousarray(cells, dtype=np.int64)
        angle = np.ascontiguousarray(np.broadcast_to(np.asarray(angle, dtype=np.float64), cells.shape))
        cases.append(dict(name=name, z=z, de=float(de), cells=cells, angle=angle, h=h, w=w, D=D,
                          ages=np.asarray(kt, dtype=np.float64), delta=delta, min_samples=ms))

    rng = np.random.default_rng(20261017)
    z = pr.synthetic_z(600)
    on = pr.scarp_cells(600, 40, rng, spread=3.0)
    ang = 0.2 + 0.05 * rng.standard_normal(40)
    add("synthetic h100 w0 D8", z, 1.0, on, ang, 100, 0, 8, ages[:NA["synthetic h100 w0 D8"]], ms=15)
    add("synthetic h100 w5 D1", z, 1.0, on, ang, 100, 5, 1, ages[:NA["synthetic h100 w5 D1"]], ms=15)
    add("synthetic h30 w5 D4", z, 1.0, on, ang, 30, 5, 4, ages[:NA["synthetic h30 w5 D4"]], ms=15)
    add("64 ages", z, 1.0, on[:12], 0.2, 100, 2, 3, 10 ** np.linspace(0, NA["64 ages"], 64), ms=15)
    add("one age", z, 1.0, on[:30], 0.2, 100, 2, 8, [10.0], ms=15)
    add("repeated cells", z, 1.0, np.repeat(on[:5], 3)[::-1], 0.2, 100, 5, 4, ages[:NA["repeated cells"]], ms=15, delta=0.0)
    # the whole range the call accepts: D = h - min_samples, which leaves a shifted step min_samples points of one side
    add("D = h - min_samples", z, 1.0, on[:20], 0.2, 12, 1, 8, ages[:NA["D = h - min_samples"]], ms=4)
    add("no cell", z, 1.0, on[:0], 0.2, 100, 5, 8, ages, ms=15)
    n = 300
    zb = pr.synthetic_z(n, seed=7)
    edge = np.concatenate([np.array([0, n - 1, n * (n - 1), n * n - 1]), rng.integers(0, n, 8), rng.integers(0, n, 8) * n,
                           rng.integers(0, n, 8) * n + n - 1, (n - 1) * n + rng.integers(0, n, 8),
                           rng.integers(0, 40, 16) * n + rng.integers(0, n, 16),
                           rng.integers(0, n, 16) * n + rng.integers(n - 40, n, 16)])
    add("borders and corners", zb, 1.0, edge, rng.uniform(-np.pi, np.pi, len(edge)), 100, 5, 3, ages[:NA["borders and corners"]], ms=20)
    zn = pr.synthetic_z(400, seed=11).copy()
    zn[rng.random(zn.shape) < 0.004] = np.nan
    zn[180:200, 150:230] = np.nan
    add("NaN cells", zn, 1.0, rng.integers(0, zn.size, 60), rng.uniform(-np.pi / 2, np.pi / 2, 60), 40, 3, 3,
        ages[:NA["NaN cells"]], ms=20)
    return cases


def segment_cases():
    """The segment cases: the fields of profile_cases plus labels and min_profiles."""
    from scarplet_amd import _plan
    ages = _plan.age_grid()
    cases = []

    def add(name, z, de, cells, labels, angle, h, w, D, kt, delta=1.0, ms=4, mp=1):
        cells = np.ascontiguousarray(cells, dtype=np.int64)
        angle = np.ascontiguousarray(np.broadcast_to(np.asarray(angle, dtype=np.float64), cells.shape))
        cases.append(dict(name=name, z=z, de=float(de), cells=cells, labels=np.asarray(labels, dtype=np.int64), angle=angle,
                          h=h, w=w, D=D, ages=np.asarray(kt, dtype=np.float64), delta=delta, min_samples=ms, min_profiles=mp))

    rng = np.random.default_rng(20261018)
    z = pr.synthetic_z(600)
    on = pr.scarp_cells(600, 40, rng, spread=3.0)
    ang = 0.2 + 0.05 * rng.standard_normal(40)
    lab = rng.integers(1, 5, 40) * 3                                      # four segments, their cells interleaved
    add("segments h100 w0 D8", z, 1.0, on, lab, ang, 100, 0, 8, ages[:NA["synthetic h100 w0 D8"]], ms=15)
    add("segments h30 w5 D4", z, 1.0, on, lab, ang, 30, 5, 4, ages[:NA["synthetic h30 w5 D4"]], ms=15)
    # segments of 1, 2, 64, 65 and 300 cells in one call: both sides of the 64-profile block of the segmented sum, and
    # several blocks.  Short profiles and two young ages
    sizes = [1, 2, 64, 65, 300]
    lab = np.repeat([5, 1, 9, 2, 7], sizes)
    big = pr.scarp_cells(600, len(lab), rng, spread=1.0)
    add("sizes 1 2 64 65 300", z, 1.0, big, lab, 0.2 + 0.02 * rng.standard_normal(len(lab)), 6, 1, 2, [1.0, 3.0], ms=3)
    perm = rng.permutation(len(lab))[:150]                                # the same cells, fewer, in shuffled order
    add("shuffled order", z, 1.0, big[perm], lab[perm], 0.2, 30, 2, 3, ages[:NA["shuffled order"]:2], ms=10, delta=4.0)
    # the corners at orientation 0 have nothing on one side: a segment none of whose cells is usable, next to one that is
    n = 300
    zb = pr.synthetic_z(n, seed=7)
    corners = np.array([0, n - 1, n * (n - 1), n * n - 1, 150 * n + 150, 151 * n + 150])
    add("unusable segment", zb, 1.0, corners, [4, 4, 4, 4, 6, 6], 0.0, 100, 5, 3, ages[:NA["unusable segment"]], ms=20)
    add("no cell", z, 1.0, on[:0], on[:0], 0.2, 100, 5, 8, ages, ms=15)
    # 217 rows of 64 ages are 111 KB: past the 64 KB up to which the kernels stage the erf table in LDS, so the residual and
    # choice kernels read it from global memory.  Segments of 1, 64 and 65 cells (a rng of its own: the cases above stay)
    rng = np.random.default_rng(20261019)
    lab = np.repeat([2, 3, 1], [1, 64, 65])
    add("table in global memory", pr.synthetic_z(256), 1.0, pr.scarp_cells(256, len(lab), rng, spread=1.0), lab,
        0.2 + 0.02 * rng.standard_normal(len(lab)), 100, 1, 4, 10 ** np.linspace(0, NA["64 ages"], 64), ms=15)
    return cases


# how far each case's age grid goes (the number of default ages, or the exponent of the last of the 64): chosen on the
# CPU so that no compared (age, shift) passes COND_MAX - a shift towards the profile's end leaves the erf column nearly
# linear over the profile sooner than the centred one (docs/profiles.md, "The centre shift")
NA = {"synthetic h100 w0 D8": 35, "synthetic h100 w5 D1": 35, "synthetic h30 w5 D4": 35, "64 ages": 3.4, "repeated cells": 35,
      "D = h - min_samples": 32, "borders and corners": 35, "NaN cells": 35, "shuffled order": 24, "unusable segment": 35}
