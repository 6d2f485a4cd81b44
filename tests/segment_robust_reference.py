"""numpy restatements of sc_fit_segments_robust (docs/segments.md, "Weights and robust fits"; include/scarplet_hip.h).

Two of them, run through all the iterates each on its own.  ``joint_lstsq``: per age and iterate ONE ``np.linalg.lstsq`` in
float64 on the full weighted design matrix of the active profiles - a dummy intercept and a dummy slope column per
profile plus the shared erf column, 2 m + 1 columns, equilibrated as ``robust_reference.wfit`` equilibrates (every
profile's data less its weighted mean, every column at unit norm) - never the per-profile orthogonalisation the device
uses; dormant profiles are frozen.  ``joint_fw``: the Frisch-Waugh form (each profile's erf column and data orthogonalised
against its own weighted (1, s), then one ratio of sums) in ``np.longdouble``.  Their difference is the reference's own
error (tests/test_segment_robust_host.py).  The samples are ``robust_reference.sample_weighted``'s, the factors, rho and
the choice ``robust_reference``'s, the grouping ``segment_reference``'s."""
import numpy as np
from scipy.special import erf

import profile_reference as pr
import robust_reference as rr
import segment_reference as sr
from profile_reference import RTOL, COND_MAX, TIE_SHARE      # noqa: F401

ROW_FLOATS = sr.ROW_FLOATS + ("loss", "scale")
ROW_INTS = sr.ROW_INTS
MAD = rr.MAD


# ---- the joint weighted fit of one age ----------------------------------------------------------------------------------
def _see(s, e, Q):
    """sum_c See_c of the weighted columns in float64: what decides whether an age is dead."""
    W = Q.sum(axis=1)
    sc = s[None, :] - ((Q * s).sum(axis=1) / W)[:, None]
    ec = e[None, :] - ((Q * e).sum(axis=1) / W)[:, None]
    e2 = ec - ((Q * sc * ec).sum(axis=1) / (Q * sc * sc).sum(axis=1))[:, None] * sc
    return float((Q * e2 * e2).sum())


def joint_lstsq(s, P, e, Q):
    """(c0 (m), b (m), a, sum See, condition number) of one age for the m active profiles P (m x np, 0 where a point is
    missing) under the weights Q (m x np, 0 where a point is missing or weighs nothing): float64 lstsq on the rows scaled by
    sqrt(q), rows of weight 0 left out."""
    m, npts = P.shape
    g = np.sqrt(Q)
    pm = (Q * P).sum(axis=1) / Q.sum(axis=1)
    keep = Q > 0
    rows = int(keep.sum())
    X = np.zeros((rows, 2 * m + 1))
    y = np.zeros(rows)
    o = 0
    for c in range(m):
        k = keep[c]
        n = int(k.sum())
        X[o:o + n, 2 * c] = g[c, k]
        X[o:o + n, 2 * c + 1] = g[c, k] * s[k]
        X[o:o + n, -1] = g[c, k] * e[k]
        y[o:o + n] = (P[c, k] - pm[c]) * g[c, k]
        o += n
    norm = np.linalg.norm(X, axis=0)
    coef, _, rank, sv = np.linalg.lstsq(X / norm, y, rcond=None)
    assert rank == X.shape[1], (rank, X.shape)
    coef = coef / norm
    return coef[0:-1:2] + pm, coef[1:-1:2], float(coef[-1]), _see(s, e, Q), float(sv[0] / sv[-1])


def joint_fw(s, P, e, Q):
    """The same fit in the Frisch-Waugh form in np.longdouble (e itself is scipy's float64)."""
    L = np.longdouble
    s, P, e, Q = s.astype(L), P.astype(L), e.astype(L), Q.astype(L)
    W = Q.sum(axis=1)
    sbar, pbar, ebar = (Q * s).sum(axis=1) / W, (Q * P).sum(axis=1) / W, (Q * e).sum(axis=1) / W
    sc = s[None, :] - sbar[:, None]
    sss = (Q * sc * sc).sum(axis=1)
    beta = (Q * sc * (P - pbar[:, None])).sum(axis=1) / sss
    gamma = (Q * sc * (e[None, :] - ebar[:, None])).sum(axis=1) / sss
    e2 = (e[None, :] - ebar[:, None]) - gamma[:, None] * sc
    p2 = (P - pbar[:, None]) - beta[:, None] * sc
    see = (Q * e2 * e2).sum()
    a = (Q * e2 * p2).sum() / see
    b = beta - a * gamma
    c0 = pbar - a * ebar - b * sbar
    return c0, b, a, see, 0.0


# ---- one segment ----------------------------------------------------------------------------------------------------------
def fit_segment(z, wt, de, cells, sa, ca, h, w, ages, delta=1.0, min_samples=4, min_profiles=1, robust=None, tuning=None,
                iterations=8, robust_scale=None, fit=joint_lstsq, force_ls=None):
    """One segment's row as a dict: the fields of sc_segment_robust_fit, plus - per age - 'curve' (the loss), 'sse_curve',
    'sse0' (the curve of iterate 0), 'A' (a), 'C0' and 'B' (A x n_profiles), 'per_loss', 'per_sse', 'per_down' and 'dorm'
    (A x n_profiles: each usable profile's share, its down-weighted points, whether it was dormant in the last iterate),
    and 'cond', 'ptp', 'used', 'cell_n' as segment_reference.fit_segment has them.  ``force_ls`` takes ls_index as given."""
    ny, nx = z.shape
    nA = len(ages)
    j = np.arange(-h, h + 1)
    neg, pos = j < 0, j > 0
    prof, wts, used, cell_n = [], [], [], []
    for k, cell in enumerate(cells):
        r_, c_ = divmod(int(cell), nx)
        p, u = rr.sample_weighted(z, wt, float(r_), float(c_), sa[k], ca[k], h, w)
        ok = ~np.isnan(p)
        cell_n.append(int(ok.sum()))
        good = int((ok & neg).sum()) >= min_samples and int((ok & pos).sum()) >= min_samples
        used.append(int(good))
        if good:
            prof.append(p)
            wts.append(u)
    m = len(prof)
    n = int(sum(int((~np.isnan(p)).sum()) for p in prof))
    row = {"n_cells": len(cells), "n_profiles": m, "n": n, "dof": n - 2 * m - 1, "kt_index": -1, "lo_index": -1,
           "hi_index": -1, "status": 1, "n_down": 0, "ls_index": -1, "n_dormant": 0, "curve": np.full(nA, np.nan),
           "sse0": np.full(nA, np.nan), "cond": 0.0, "ptp": np.nan, "used": np.array(used, dtype=np.int64),
           "cell_n": np.array(cell_n, dtype=np.int64)}
    for f in ROW_FLOATS:
        row[f] = np.nan
    if m < min_profiles or row["dof"] < 1:
        return row
    F = np.float64 if fit is joint_lstsq else np.longdouble
    V = ~np.isnan(np.array(prof))
    P = np.where(V, np.array(prof), 0.0)
    U = np.where(V, np.array(wts), 0.0)
    s = j.astype(np.float64) * de
    E = [erf(s / (2 * np.sqrt(kt))) for kt in ages]
    dof = row["dof"]

    def resid(c0, b, a, e):
        return P.astype(F) - ((c0[:, None] + b[:, None] * s.astype(F)[None, :]) + a * e.astype(F)[None, :])

    # iterate 0: the weighted least squares fit of every age, every usable profile active
    conds = []
    C0, B, Aa, R = [], [], [], []
    for e in E:
        c0, b, a, _, cd = fit(s, P, e, U)
        conds.append(cd)
        C0.append(np.array(c0, dtype=F)); B.append(np.array(b, dtype=F)); Aa.append(a); R.append(resid(c0, b, a, e))
    sse0 = np.array([float((U * r * r).sum()) for r in R])
    row["sse0"] = sse0
    if np.isnan(sse0).all():
        row["status"] = 1 | 32
        return row
    ls = int(np.argmin(np.where(np.isnan(sse0), np.inf, sse0))) if force_ls is None else int(force_ls)
    curve, sigma, flag = sse0, np.nan, 0
    per_loss = np.array([np.asarray((U * r * r).sum(axis=1), dtype=np.float64) for r in R])
    per_sse = per_loss.copy()
    per_down = np.zeros((nA, m), dtype=np.int64)
    dorm = np.zeros((nA, m), dtype=bool)
    if robust is not None:
        k = float(tuning) if tuning is not None else (rr.HUBER_K if robust == "huber" else rr.TUKEY_K)
        if robust_scale is not None:
            sigma = float(robust_scale)
        else:
            sigma = float(MAD * np.sort(np.abs(R[ls][V]).astype(np.float64))[(n - 1) // 2])
        if not sigma > 0:
            flag = 16
        else:
            c = k * sigma
            curve = np.full(nA, np.nan)
            for i, e in enumerate(E):
                c0, b, a, r = C0[i].copy(), B[i].copy(), Aa[i], R[i]
                dead = False
                idle = np.zeros(m, dtype=bool)
                for _ in range(iterations):
                    with np.errstate(invalid="ignore", divide="ignore"):
                        Q = U * rr.factor(robust, r.astype(np.float64), c)
                    idle = (((Q > 0) & neg[None, :]).sum(axis=1) < min_samples) | (((Q > 0) & pos[None, :]).sum(axis=1) < min_samples)
                    act = ~idle
                    if not act.any():
                        dead = True
                        break
                    c0a, ba, a, see, cd = fit(s, P[act], e, Q[act])
                    if not see > 0:
                        dead = True
                        break
                    conds.append(cd)
                    c0[act], b[act] = c0a, ba                  # a dormant profile keeps its own
                    r = resid(c0, b, a, e)
                if dead:
                    C0[i], B[i], Aa[i] = np.full(m, np.nan), np.full(m, np.nan), np.nan
                    per_loss[i], per_sse[i] = np.nan, np.nan
                    continue
                C0[i], B[i], Aa[i] = c0, b, a
                per_loss[i] = np.asarray((U * rr.rho(robust, r, F(c))).sum(axis=1), dtype=np.float64)
                per_sse[i] = np.asarray((U * r * r).sum(axis=1), dtype=np.float64)
                per_down[i] = ((rr.factor(robust, r.astype(np.float64), c) < 1) & V).sum(axis=1)
                dorm[i] = idle
                curve[i] = float(per_loss[i].sum())
            if np.isnan(curve).all():
                row["status"] = 1 | 32
                row["scale"] = sigma
                return row
    best, lo, hi, status = rr.choose(curve, dof + 3, delta)
    sse_curve = per_sse.sum(axis=1)
    row.update(kt_index=best, lo_index=lo, hi_index=hi, status=status | flag, kt=float(ages[best]), kt_lo=float(ages[lo]),
               kt_hi=float(ages[hi]), a=float(Aa[best]), sse=float(sse_curve[best]), loss=float(curve[best]),
               rmse=float(np.sqrt(curve[best] / dof)), scale=sigma, n_down=int(per_down[best].sum()), ls_index=ls,
               n_dormant=int(dorm[best].sum()), curve=curve, sse_curve=sse_curve,
               A=np.array([float(v) for v in Aa]), C0=np.array(C0, dtype=np.float64), B=np.array(B, dtype=np.float64),
               per_loss=per_loss, per_sse=per_sse, per_down=per_down, dorm=dorm, cond=max(conds),
               ptp=max(float(p[v].max() - p[v].min()) for p, v in zip(P, V)))
    return row


def fit_segments(z, wt, de, cells, labels, angle, h, w, ages, fit=joint_lstsq, **kw):
    """Rows (a list of dicts, one per distinct positive label in ascending order, each with 'label' and 'where': the input
    positions of its cells)."""
    z = np.asarray(z, dtype=np.float64)
    wt = None if wt is None else np.asarray(wt, dtype=np.float64)
    ages = np.asarray(ages, dtype=np.float64)
    cells = np.asarray(cells)
    angle = np.broadcast_to(np.asarray(angle, dtype=np.float64), (len(cells),))
    sa, ca = np.sin(angle), np.cos(angle)
    lab, where = sr.group(labels)
    rows = []
    for l, pos in zip(lab, where):
        row = fit_segment(z, wt, de, cells[pos], sa[pos], ca[pos], h, w, ages, fit=fit, **kw)
        row["label"], row["where"] = int(l), pos
        rows.append(row)
    return rows


def restate(c, fit=joint_lstsq):
    return fit_segments(c["z"], c["weights"], c["de"], c["cells"], c["labels"], c["angle"], c["h"], c["w"], c["ages"], fit=fit,
                        delta=c["delta"], min_samples=c["min_samples"], min_profiles=c["min_profiles"], **c["robust"])


# ---- comparing the tables with a restatement ----------------------------------------------------------------------------------
def tables_of(rows, n_cells, n_ages):
    """A restatement's rows as (table, cell table indexed by input position, curves): lists of dicts and arrays shaped as
    compare takes the device's - what sets one restatement against the other."""
    table, curve = [], np.full((len(rows), n_ages), np.nan)
    ct = np.zeros(n_cells, dtype=[("used", np.int64), ("n", np.int64), ("b", np.float64), ("c0", np.float64), ("sse", np.float64),
                                  ("loss", np.float64), ("n_down", np.int64), ("dormant", np.int64), ("label", np.int64)])
    for f in ("b", "c0", "sse", "loss"):
        ct[f] = np.nan
    for s, r in enumerate(rows):
        g = {f: r[f] for f in ("label",) + ROW_INTS + ROW_FLOATS + ("kt_index", "lo_index", "hi_index", "status", "n_down",
                                                                   "ls_index", "n_dormant")}
        g["height"] = 2.0 * r["a"]
        table.append(g)
        pos = r["where"]
        ct["used"][pos], ct["n"][pos], ct["label"][pos] = r["used"], r["cell_n"], r["label"]
        if r["status"] & 1:
            continue
        curve[s] = r["curve"]
        up, gi = pos[r["used"] == 1], r["kt_index"]
        ct["b"][up], ct["c0"][up] = r["B"][gi], r["C0"][gi]
        ct["sse"][up], ct["loss"][up] = r["per_sse"][gi], r["per_loss"][gi]
        ct["n_down"][up], ct["dormant"][up] = r["per_down"][gi], r["dorm"][gi]
    return table, ct, curve


def compare(case, ref, table, cell_table, curve):
    """The device's tables (rows in label order, the cell table indexed by input position, the (S, A) loss curves) against
    ``ref`` (restate(case)), in the manner of segment_reference.compare and robust_reference.compare_rows: the loss, the
    sse, the curve, each profile's share and the scale relative, the coefficients over the largest range of a profile;
    the counts exact; the indices equal except for ties decided inside RTOL (a segment whose ls_index was such a tie is
    compared with the restatement at the device's ls_index); n_down, n_dormant, the per-cell flags and the status exact
    where there is no tie.  Returns the figures."""
    h, de, delta = case["h"], case["de"], case["delta"]
    out = {"segments": len(ref), "fitted": 0, "ties": 0, "loss": 0.0, "coef": 0.0, "scale": 0.0, "cond": 0.0}
    assert len(table) == len(ref)
    sa, ca = np.sin(case["angle"]), np.cos(case["angle"])
    for s, (r, g) in enumerate(zip(ref, table)):
        L = r["label"]
        assert int(g["label"]) == L
        for f in ROW_INTS:
            assert int(g[f]) == r[f], (L, f, g[f], r[f])
        ct = cell_table[r["where"]]
        assert np.array_equal(ct["used"], r["used"]) and np.array_equal(ct["n"], r["cell_n"]), L
        assert np.all(ct["label"] == L)
        assert (int(g["status"]) & 33) == (r["status"] & 33), (L, g["status"], r["status"])
        if r["status"] & 1:
            assert int(g["kt_index"]) == -1 and int(g["lo_index"]) == -1 and int(g["hi_index"]) == -1, L
            assert int(g["ls_index"]) == -1 and int(g["n_down"]) == 0 and int(g["n_dormant"]) == 0, L
            assert all(np.isnan(g[f]) for f in ROW_FLOATS if f != "scale") and np.isnan(g["height"]), L
            if np.isnan(r["scale"]):
                assert np.isnan(g["scale"]), L
            else:
                assert abs(float(g["scale"]) - r["scale"]) <= RTOL * r["scale"], (L, g["scale"], r["scale"])
            assert np.isnan(curve[s]).all()
            assert all(np.isnan(ct[f]).all() for f in ("b", "c0", "sse", "loss")), L
            assert (ct["n_down"] == 0).all() and (ct["dormant"] == 0).all(), L
            continue
        out["fitted"] += 1
        tie = False
        if int(g["ls_index"]) != r["ls_index"]:
            m0 = r["sse0"][r["ls_index"]]
            assert abs(r["sse0"][int(g["ls_index"])] - m0) <= RTOL * m0, (L, "ls_index", g["ls_index"], r["ls_index"])
            tie = True
            pos = r["where"]
            r2 = fit_segment(case["z"], case["weights"], de, case["cells"][pos], sa[pos], ca[pos], h, case["w"], case["ages"],
                             delta=delta, min_samples=case["min_samples"], min_profiles=case["min_profiles"],
                             force_ls=int(g["ls_index"]), **case["robust"])
            r2["label"], r2["where"] = L, pos
            r = r2
        assert r["cond"] <= COND_MAX, ("the inputs leave the tolerance's ground", L, r["cond"])
        out["cond"] = max(out["cond"], r["cond"])
        assert (int(g["status"]) & 16) == (r["status"] & 16), (L, g["status"], r["status"])
        cv, dof = r["curve"], r["dof"]
        gi, glo, ghi = int(g["kt_index"]), int(g["lo_index"]), int(g["hi_index"])
        if gi != r["kt_index"]:
            assert abs(cv[gi] - r["loss"]) <= RTOL * r["loss"], (L, gi, r["kt_index"], cv[gi], r["loss"])
            tie = True
        thr = cv[gi] * (1.0 + delta / dof)
        for gv, rv, i in ((glo, r["lo_index"], max(glo, r["lo_index"]) - 1), (ghi, r["hi_index"], min(ghi, r["hi_index"]) + 1)):
            if gv != rv:
                assert abs(cv[i] - thr) <= RTOL * thr, (L, gv, rv, cv[i], thr)
                tie = True
        u = r["used"] == 1
        if tie:
            out["ties"] += 1
        else:
            assert int(g["status"]) == r["status"], (L, g["status"], r["status"])
            assert int(g["n_down"]) == int(r["per_down"][gi].sum()), (L, g["n_down"], r["n_down"])
            assert int(g["n_dormant"]) == int(r["dorm"][gi].sum()), (L, g["n_dormant"], r["n_dormant"])
            assert np.array_equal(ct["n_down"][u], r["per_down"][gi]), L
            assert np.array_equal(ct["dormant"][u], r["dorm"][gi].astype(np.int64)), L
        gc = np.asarray(curve[s], dtype=np.float64)
        assert np.array_equal(np.isnan(gc), np.isnan(cv)), (L, "NaN ages")
        live = ~np.isnan(cv)
        dl = float(np.max(np.abs(gc[live] - cv[live]) / cv[live]))
        dl = max(dl, abs(float(g["loss"]) - cv[gi]) / cv[gi], abs(float(g["sse"]) - r["sse_curve"][gi]) / r["sse_curve"][gi])
        for f in ("b", "c0", "sse", "loss"):
            assert np.isnan(ct[f][~u]).all(), (L, f)
        assert (ct["n_down"][~u] == 0).all() and (ct["dormant"][~u] == 0).all(), L
        # each profile's share of the pooled sums, against the pooled sums
        dl = max(dl, float(np.max(np.abs(ct["loss"][u] - r["per_loss"][gi]))) / cv[gi],
                 float(np.max(np.abs(ct["sse"][u] - r["per_sse"][gi]))) / r["sse_curve"][gi])
        dc = max(abs(float(g["a"]) - r["A"][gi]), float(np.max(np.abs(ct["c0"][u] - r["C0"][gi]))),
                 float(np.max(np.abs(ct["b"][u] - r["B"][gi]))) * h * de) / r["ptp"]
        dsig = 0.0
        if not np.isnan(r["scale"]):
            dsig = abs(float(g["scale"]) - r["scale"]) / r["scale"] if r["scale"] > 0 else abs(float(g["scale"]))
        else:
            assert np.isnan(g["scale"]), L
        assert dl <= RTOL, (L, "loss", dl)
        assert dc <= RTOL, (L, "coefficients", dc)
        assert dsig <= RTOL, (L, "scale", dsig)
        out["loss"], out["coef"], out["scale"] = max(out["loss"], dl), max(out["coef"], dc), max(out["scale"], dsig)
    assert out["ties"] <= TIE_SHARE * max(1, out["segments"]), out
    return out


# ---- cases ----------------------------------------------------------------------------------------------------------------------
TRENCH_SEEDS = (20261019, 1, 2, 3)
TRUE_INDEX = 10
BLOCK_GPU_INDEX = 4                                                    # the true age among the ages of the GPU tests' block case


def case(name, z, de, cells, labels, angle, h, w, ages=None, delta=1.0, ms=4, mp=1, weights=None, **robust):
    from scarplet_amd import _plan
    cells = np.ascontiguousarray(cells, dtype=np.int64)
    angle = np.ascontiguousarray(np.broadcast_to(np.asarray(angle, dtype=np.float64), cells.shape))
    labels = np.ascontiguousarray(np.broadcast_to(np.asarray(labels, dtype=np.int64), cells.shape))
    return dict(name=name, z=z, de=float(de), cells=cells, labels=labels, angle=angle, h=h, w=w,
                ages=np.asarray(_plan.age_grid() if ages is None else ages, dtype=np.float64), delta=delta, min_samples=ms,
                min_profiles=mp, weights=weights, robust=robust)


def _across(n=600, theta=0.2):
    """Columns from the scarp line of synthetic_scarp(n), per cell."""
    row, col = np.arange(n, dtype=np.float64)[:, None], np.arange(n, dtype=np.float64)[None, :]
    return col - (n / 2 + (row - n / 2) * np.tan(theta)), row


def trench_surface(seed):
    """(z, cells, cc): synthetic_z(600) with a trench of depth 0.8 and Gaussian width 4 cells dug 15 cells to the right of
    the scarp line on rows 0..399, and noise 0.05 from default_rng(seed) - which gives the cells first."""
    rng = np.random.default_rng(seed)
    cells = pr.scarp_cells(600, 100, rng)
    cc, row = _across()
    z = pr.synthetic_z(600)
    z = z - 0.8 * np.exp(-((cc - 15.0) / 4.0) ** 2 / 2.0) * (row < 400) + 0.05 * rng.standard_normal(z.shape)
    return z, cells, cc


def trench_case(seed=TRENCH_SEEDS[0], mask=False, **robust):
    """100 cells of the scarp line as ONE segment, h = 100, w = 2, min_samples = 15, the default 35 ages.  ``mask``: a 0 / 1
    weight plane with the trench's strip (3 widths either side) taken out."""
    z, cells, cc = trench_surface(seed)
    wt = np.where(np.abs(cc - 15.0) <= 12.0, 0.0, 1.0) if mask else None
    return case("trench", z, 1.0, cells, 1, 0.2, 100, 2, ms=15, weights=wt, **robust)


def block_case(n_cells=100, ages=None, **robust):
    """The trench's surface without the trench (seed 20261019), +5.0 on rows 200..211 to the right of the scarp: the
    profiles that cross the block lose one whole side under Tukey and go dormant.  ``n_cells``: the first so many of the
    100 cells; ``ages``: None for the default 35."""
    rng = np.random.default_rng(TRENCH_SEEDS[0])
    cells = pr.scarp_cells(600, 100, rng)[:n_cells]
    cc, row = _across()
    z = pr.synthetic_z(600) + 0.05 * rng.standard_normal((600, 600))
    z = z + 5.0 * ((row >= 200) & (row <= 211) & (cc > 3))
    return case("block", z, 1.0, cells, 1, 0.2, 100, 2, ages=ages, ms=15, **robust)


def gpu_cases(loss):
    """The cases of one loss ("huber" or "tukey") of tests/test_gpu_segment_robust.py, by name.  Seeded: the same on every
    box.  Small: the restatement's matrix has 2 m + 1 columns."""
    rng = np.random.default_rng(20261019)
    out = {}

    def add(name, *a, **kw):
        kw.setdefault("robust", loss)
        out[name] = case(name, *a, **kw)

    z = pr.synthetic_z(600)
    # the blocked sum's edges: segments of 1, 2, 63, 64, 65 and 129 usable profiles, with cells that are not usable (the
    # grid's corners: nothing on one side) among them.  Short profiles and six young ages keep the restatement quick
    sizes = [1, 2, 63, 64, 65, 129]
    labs = [5, 1, 9, 2, 7, 4]
    on = pr.scarp_cells(600, sum(sizes), rng, spread=1.0)
    lab = np.repeat(labs, sizes)
    corners = np.array([0, 599, 599 * 600, 600 * 600 - 1, 0, 599])
    cells = np.concatenate([on, corners])
    lab = np.concatenate([lab, [5, 1, 9, 2, 7, 4]])
    perm = rng.permutation(len(cells))
    ang = np.concatenate([0.2 + 0.02 * rng.standard_normal(len(on)), np.zeros(len(corners))])
    add("sizes 1 2 63 64 65 129", z, 1.0, cells[perm], lab[perm], ang[perm], 15, 1, ages=10 ** np.linspace(0, 1.5, 6), ms=5, iterations=3)
    few = pr.scarp_cells(600, 12, rng, spread=3.0)
    fang = 0.2 + 0.05 * rng.standard_normal(12)
    flab = np.arange(12) % 3 + 1
    for h in (31, 32, 15):                                                 # 63, 65 and 31 points: a lane round and its edges
        add("h%d" % h, z, 1.0, few, flab, fang, h, 2, ages=None if h > 15 else 10 ** np.linspace(0, 2.7, 28), ms=min(h, 15) - 3, iterations=4)
    add("one age", z, 1.0, few, flab, fang, 100, 2, ages=[10.0], ms=15, iterations=5)
    add("64 ages", z, 1.0, few, flab, fang, 100, 2, ages=10 ** np.linspace(0, 3.4, 64), ms=15, iterations=3)   # the table in global memory
    add("no cell", z, 1.0, few[:0], flab[:0], 0.2, 100, 5, ms=15, iterations=2)
    add("labels <= 0 only", z, 1.0, few[:5], [0, -1, 0, 0, -7], 0.2, 100, 5, ms=15, iterations=2)
    # segments that are not fitted: one with fewer usable profiles than min_profiles, one none of whose cells is usable
    add("not fitted", z, 1.0, np.concatenate([few, [0, 599]]), np.concatenate([np.repeat([1, 2], [9, 3]), [3, 3]]),
        np.concatenate([fang, [0.0, 0.0]]), 100, 2, ms=15, mp=5, iterations=3)
    parent = {c["name"]: c for c in sr.gpu_cases()}
    for name in ("borders", "NaN cells"):
        p = parent[name]
        add(name, p["z"], p["de"], p["cells"], p["labels"], p["angle"], p["h"], p["w"], ages=p["ages"], delta=p["delta"],
            ms=p["min_samples"], mp=p["min_profiles"], iterations=3)
    on = pr.scarp_cells(600, 40, rng, spread=3.0)
    ang = 0.2 + 0.05 * rng.standard_normal(40)
    lab = rng.integers(1, 5, 40) * 2
    add("robust_scale given", z, 1.0, on, lab, ang, 100, 2, ms=15, robust_scale=0.08, tuning=2.0, iterations=6)
    if loss == "tukey":                                                    # every point beyond c at once: status 1 | 32
        add("no age survives", z, 1.0, on[:8], lab[:8], ang[:8], 100, 2, ms=15, robust_scale=1e-9, iterations=2)
    # the weight planes of robust_reference.gpu_cases: a 0 / 1 plane that masks a strip beside the scarp line, a random
    # positive plane, one with NaN cells scattered and in a block - and weights alone
    cc, _ = _across()
    strip = np.where((cc > 20) & (cc < 32), 0.0, 1.0) * np.ones((600, 600))
    add("weights: a strip of zeros", z, 1.0, on, lab, ang, 100, 2, ms=15, weights=strip, iterations=4)
    add("weights: random positive", z, 1.0, on, lab, ang, 60, 3, ms=15, weights=rng.uniform(0.2, 3.0, z.shape), iterations=4)
    holes = rng.uniform(0.5, 1.5, z.shape)
    holes[rng.random(z.shape) < 0.004] = np.nan
    holes[280:300, 250:330] = np.nan
    add("weights: NaN cells", z, 1.0, on, lab, ang, 60, 3, ms=15, weights=holes, iterations=4)
    add("weights alone", z, 1.0, on, lab, ang, 60, 3, ms=15, weights=rng.uniform(0.2, 3.0, z.shape), robust=None)
    # (half the cells and the nine ages around the true one, index 4 here: the restatement's matrix stays small)
    from scarplet_amd import _plan
    b = block_case(n_cells=50, ages=_plan.age_grid()[6:15], robust=loss, iterations=4)
    out[b["name"]] = b
    return out
