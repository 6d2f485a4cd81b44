"""numpy restatement of sc_channel_segments (docs/channels.md, "One width per reach"; include/scarplet_hip.h),
algebraically independent of the device's route.  Stage one is ``channel_reference.cell_pairs``: a float64 ``lstsq`` for EACH
(cell, frequency, shift) and the first smallest sse in the order tried.  Given those shifts, every (reach, frequency) is ONE
float64 ``lstsq`` on the full, column-scaled design matrix - ``2 m + 1`` columns with ``depth="segment"`` (an intercept and a
slope per profile, one shared Gaussian column), block-diagonal ``3 m`` columns with ``depth="profile"``.  A second
restatement of the joint fit in ``np.longdouble`` on the per-profile orthogonalised form is the reference-side noise floor.
Whether a pair is dead is decided in float64 for both (``channel_reference.see64``)."""
import numpy as np

import channel_reference as cr
import shift_reference as sh

RTOL, COND_MAX, TIE_SHARE = cr.RTOL, cr.COND_MAX, cr.TIE_SHARE
MODES = ("profile", "segment")
ROW_INTS = ("n_cells", "n_profiles", "n", "dof")
ROW_FLOATS = ("f", "f_lo", "f_hi", "a", "sse", "rmse")
DERIVED = cr.DERIVED[:-2]
SG_BLOCK = 64


def blocked_sum(x):
    """The family's sum over the usable profiles (axis 0, input order): blocks of 64 in sequence from the first term, then
    the block sums in sequence.  One profile is no addition at all; NaN propagates."""
    x = np.asarray(x)
    parts = []
    for r0 in range(0, len(x), SG_BLOCK):
        acc = x[r0].copy()
        for r in range(r0 + 1, min(len(x), r0 + SG_BLOCK)):
            acc = acc + x[r]
        parts.append(acc)
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    return acc


# ---- stage one ----------------------------------------------------------------------------------------------------------------
def stage_cell(z, de, cell, sa, ca, h, w, D, freqs, min_samples):
    """``channel_reference.cell_pairs`` of one cell and, where usable: 'p', 'j' (the valid points), 'pick' (the rank of the
    chosen shift of every frequency), 'shifts' (d_ci; 0 where the frequency is dead), 'curve' (sse*_ci, NaN where dead) and
    'dmargin' (per live frequency, how far the runner-up shift is above the chosen one, relative to the chosen sse)."""
    c = cr.cell_pairs(z, de, cell, sa, ca, h, w, D, freqs, min_samples)
    if not c["usable"]:
        return c
    p, j, _, _ = sh.profile_of(z, cell, sa, ca, h, w, min_samples)
    F = len(freqs)
    g = np.where(np.isnan(c["grid"]), np.inf, c["grid"])
    pick = np.argmin(g, axis=1)
    curve = c["grid"][np.arange(F), pick]
    srt = np.sort(g, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        dm = (srt[:, 1] - srt[:, 0]) / srt[:, 0] if g.shape[1] > 1 else np.full(F, np.inf)
    dm = np.where(np.isnan(curve), np.inf, dm)
    c.update(p=p, j=j, pick=pick, shifts=np.array(c["order"])[pick], curve=curve, dmargin=dm)
    return c


# ---- the joint fit of one (reach, frequency), the shifts given ----------------------------------------------------------------
def _columns(us, i, de, f):
    return [cr.gauss_column(u["j"], int(u["shifts"][i]), de, f) for u in us]


def joint_lstsq(us, i, de, f, mode):
    """One float64 lstsq on the full design matrix of the usable profiles ``us`` at frequency i, its columns scaled to length
    1: (sse, per-profile (c0, b, a) as an (m, 3) array, per-profile sse, the condition number)."""
    m = len(us)
    es = _columns(us, i, de, f)
    ns = [len(u["p"]) for u in us]
    off = np.concatenate([[0], np.cumsum(ns)])
    own = mode == "profile"
    X = np.zeros((off[-1], (3 if own else 2) * m + (0 if own else 1)))
    y = np.concatenate([u["p"] for u in us])
    k = 3 if own else 2
    for c, u in enumerate(us):
        r = slice(off[c], off[c + 1])
        s = u["j"].astype(np.float64) * de
        X[r, k * c] = 1.0
        X[r, k * c + 1] = s
        X[r, k * c + 2 if own else 2 * m] = es[c]
    norm = np.linalg.norm(X, axis=0)
    sol, _, _, sv = np.linalg.lstsq(X / norm, y, rcond=None)
    sol = sol / norm
    coefs = np.empty((m, 3))
    per = np.empty(m)
    for c, u in enumerate(us):
        s = u["j"].astype(np.float64) * de
        coefs[c] = (sol[k * c], sol[k * c + 1], sol[k * c + 2] if own else sol[2 * m])
        res = u["p"] - (coefs[c, 0] + coefs[c, 1] * s + coefs[c, 2] * es[c])
        per[c] = np.sum(res * res)
    return float(np.sum(per)), coefs, per, float(sv[0] / sv[-1])


def joint_longdouble(us, i, de, f, mode):
    """The same fit on the per-profile orthogonalised form in np.longdouble: (sse, the row's a)."""
    L = np.longdouble
    es = _columns(us, i, de, f)
    if mode == "profile":
        fits = [cr.fit_pair_longdouble(u["j"].astype(np.float64) * de, u["p"], e) for u, e in zip(us, es)]
        return sum(t[1] for t in fits), sum(t[0][2] for t in fits) / L(len(us))
    terms = []
    for u, e in zip(us, es):
        s, p, e = (u["j"].astype(np.float64) * de).astype(L), u["p"].astype(L), e.astype(L)
        n = L(len(s))
        sbar, pbar, ebar = s.sum() / n, p.sum() / n, e.sum() / n
        sc = s - sbar
        sss = (sc * sc).sum()
        beta, gamma = (sc * (p - pbar)).sum() / sss, (sc * (e - ebar)).sum() / sss
        e2, p2 = (e - ebar) - gamma * sc, (p - pbar) - beta * sc
        terms.append((s, p, e, sbar, pbar, ebar, beta, gamma, (e2 * e2).sum(), (e2 * p2).sum()))
    a = sum(t[9] for t in terms) / sum(t[8] for t in terms)
    sse = L(0)
    for s, p, e, sbar, pbar, ebar, beta, gamma, _, _ in terms:
        b = beta - a * gamma
        c0 = pbar - a * ebar - b * sbar
        res = p - (c0 + b * s + a * e)
        sse += (res * res).sum()
    return sse, a


def see_sum(us, i, de, f):
    return sum(cr.see64(u["j"].astype(np.float64) * de, e) for u, e in zip(us, _columns(us, i, de, f)))


# ---- one reach -----------------------------------------------------------------------------------------------------------------
def fit_reach(stage, de, D, freqs, mode, delta, min_profiles, longdouble=False):
    """One reach's row as a dict from the stage-one records of its cells in input order: the fields of the device's table,
    plus 'used', 'cell_n', 'curve', 'coefs' (F x m x 3; float64 route), 'per' (F x m), 'shifts' (the reach's cells x F),
    'cond', 'ptp' and 'margin' - the smallest relative margin of any decision of the reach: every d_ci of a usable profile,
    the argmin and both walks."""
    F = len(freqs)
    used = np.array([1 if c["usable"] else 0 for c in stage])
    us = [c for c in stage if c["usable"]]
    m, n = len(us), sum(c["n"] for c in us)
    dof = n - (3 + (D > 0)) * m if mode == "profile" else n - 2 * m - 1 - (m if D > 0 else 0)
    shifts = np.array([c["shifts"] if c["usable"] else np.zeros(F, dtype=np.int64) for c in stage]).reshape(len(stage), F)
    row = dict(n_cells=len(stage), n_profiles=m, n=n, dof=dof, f_index=-1, lo_index=-1, hi_index=-1, status=1, used=used,
               cell_n=np.array([c["n"] for c in stage]), curve=np.full(F, np.nan), shifts=shifts, cond=0.0,
               ptp=max([c["ptp"] for c in us], default=np.nan),
               margin=min([float(c["dmargin"].min()) for c in us], default=np.inf))
    for f in ROW_FLOATS:
        row[f] = np.nan
    if m < min_profiles or dof < 1:
        return row
    dt = np.longdouble if longdouble else np.float64
    curve, avals = np.full(F, np.nan, dtype=dt), np.full(F, np.nan, dtype=dt)
    coefs, per = np.full((F, m, 3), np.nan), np.full((F, m), np.nan)
    for i, f in enumerate(freqs):
        if any(np.isnan(c["curve"][i]) for c in us):
            continue                                                   # dead in one usable profile: dead for the reach
        if mode == "segment" and not see_sum(us, i, de, f) > 0.0:
            continue
        if longdouble:
            curve[i], avals[i] = joint_longdouble(us, i, de, f, mode)
            continue
        curve[i], coefs[i], per[i], cond = joint_lstsq(us, i, de, f, mode)
        avals[i] = coefs[i, :, 2].mean() if mode == "profile" else coefs[i, 0, 2]
        row["cond"] = max(row["cond"], cond)
    row.update(curve=curve, avals=avals, coefs=coefs, per=per)
    if np.isnan(curve.astype(np.float64)).all():
        row["status"] = 1 | 32
        return row
    c64 = curve.astype(np.float64) if not longdouble else curve
    best, lo, hi, status = cr.choose(c64, dof, delta)
    at_end = D > 0 and any(abs(int(c["shifts"][best])) == D for c in us)
    sse = curve[best]
    # the margins of the argmin and of the walks, relative to the sse
    live = np.where(np.isnan(c64), np.inf, c64).astype(np.float64)
    others = np.delete(live, best)
    mg = float((others.min() - live[best]) / live[best]) if len(others) else np.inf
    thr = float(live[best]) * (1.0 + delta / dof)
    for i in range(max(lo - 1, 0), min(hi + 1, F - 1) + 1):
        if i != best and np.isfinite(live[i]):
            mg = min(mg, abs(live[i] - thr) / thr)
    row.update(f_index=best, lo_index=lo, hi_index=hi, status=status + (8 if at_end else 0), f=float(freqs[best]),
               f_lo=float(freqs[lo]), f_hi=float(freqs[hi]), a=avals[best], sse=sse, rmse=np.sqrt(sse / dof),
               margin=min(row["margin"], mg))
    return row


def group(labels):
    """The ascending labels > 0 and, for each, the input positions of its cells in input order."""
    labels = np.asarray(labels)
    lab = np.unique(labels[labels > 0])
    return lab, [np.flatnonzero(labels == l) for l in lab]


_STAGE, _ROWS = {}, {}


def stage_of(case):
    """Stage one of a case's cells (kept: both modes, and the host and the device tests of one process, share it)."""
    if case["name"] not in _STAGE:
        sa, ca = np.sin(case["angle"]), np.cos(case["angle"])
        _STAGE[case["name"]] = [stage_cell(case["z"], case["de"], case["cells"][k], sa[k], ca[k], case["h"], case["w"], case["D"],
                                           case["frequencies"], case["min_samples"]) if case["labels"][k] > 0 else None
                                for k in range(len(case["cells"]))]
    return _STAGE[case["name"]]


def restate(case, mode, longdouble=False):
    """The restatement's rows of a case in label order, each with 'label' and 'where' (the input positions of its cells)."""
    key = (case["name"], mode, longdouble)
    if key not in _ROWS:
        st = stage_of(case)
        rows = []
        for l, pos in zip(*group(case["labels"])):
            row = fit_reach([st[k] for k in pos], case["de"], case["D"], case["frequencies"], mode, case["delta"],
                            case["min_profiles"], longdouble)
            row["label"], row["where"] = int(l), pos
            rows.append(row)
        _ROWS[key] = rows
    return _ROWS[key]


# ---- comparing the device's tables with the restatement -------------------------------------------------------------------------
def compare(ref, mode, table, cell_table, curve, shifts, kept, h, de, D):
    """The device's tables (rows in label order; the cell table and the (K_kept, F) shifts in input order of the kept cells,
    ``kept`` their input positions) against ``ref`` (restate's rows).  Integers, statuses and shifts are equal except in a
    reach whose margin is <= RTOL, which counts as a tie; floats are within RTOL, the coefficients scaled by the reach's
    largest peak-to-peak range.  Asserts; returns the figures."""
    out = {"reaches": len(ref), "fitted": 0, "ties": 0, "sse": 0.0, "coef": 0.0, "cond": 0.0, "dead": 0, "margin": np.inf}
    assert len(table) == len(ref)
    at = {int(k): q for q, k in enumerate(kept)}
    for s, (r, g) in enumerate(zip(ref, table)):
        L = r["label"]
        rows = np.array([at[int(k)] for k in r["where"]])
        ct, sp = cell_table[rows], shifts[rows]
        assert int(g["label"]) == L and np.all(ct["label"] == L)
        for f in ROW_INTS:
            assert int(g[f]) == r[f], (L, f, g[f], r[f])
        assert np.array_equal(ct["used"], r["used"]) and np.array_equal(ct["n"], r["cell_n"]), L
        u = r["used"] == 1
        assert not sp[~u].any(), (L, "shifts of cells that are not usable")
        tie = r["margin"] <= RTOL
        out["margin"] = min(out["margin"], r["margin"])
        if tie:
            out["ties"] += 1
        else:
            assert np.array_equal(sp, r["shifts"]), (L, "shifts", np.argwhere(sp != r["shifts"])[:4])
        if r["status"] & 1:
            if not tie:
                assert int(g["status"]) == r["status"], (L, g["status"], r["status"])
                assert int(g["f_index"]) == -1 and int(g["lo_index"]) == -1 and int(g["hi_index"]) == -1
                assert all(np.isnan(g[f]) for f in ROW_FLOATS + DERIVED), L
                assert np.isnan(curve[s]).all()
                assert all(np.isnan(ct[f]).all() for f in ("a", "b", "c0", "sse", "shift", "depth", "centre_row", "centre_col"))
                assert not ct["shift_index"].any()
            continue
        out["fitted"] += 1
        assert r["cond"] <= COND_MAX, ("the inputs leave the tolerance's ground", L, r["cond"])
        out["cond"] = max(out["cond"], r["cond"])
        if tie:
            continue
        cv, dof = r["curve"], r["dof"]
        dead = np.isnan(cv)
        out["dead"] += int(dead.sum())
        assert np.array_equal(np.isnan(curve[s]), dead), (L, "dead frequencies")
        gi = int(g["f_index"])
        assert (gi, int(g["lo_index"]), int(g["hi_index"]), int(g["status"])) == \
            (r["f_index"], r["lo_index"], r["hi_index"], r["status"]), (L, g, r["f_index"], r["lo_index"], r["hi_index"], r["status"])
        assert float(g["f"]) == r["f"] and float(g["f_lo"]) == r["f_lo"] and float(g["f_hi"]) == r["f_hi"]
        ds = max(abs(float(g["sse"]) - cv[gi]) / cv[gi], float(np.max(np.abs(curve[s][~dead] - cv[~dead]) / cv[~dead])))
        coef = r["coefs"][gi]
        assert all(np.isnan(ct[f][~u]).all() for f in ("a", "b", "c0", "sse")) and not ct["shift_index"][~u].any(), L
        assert np.array_equal(ct["shift_index"][u], r["shifts"][u, gi]), L
        dc = max(abs(float(g["a"]) - r["a"]), float(np.max(np.abs(ct["c0"][u] - coef[:, 0]))),
                 float(np.max(np.abs(ct["b"][u] - coef[:, 1]))) * h * de, float(np.max(np.abs(ct["a"][u] - coef[:, 2])))) / r["ptp"]
        ds = max(ds, float(np.max(np.abs(ct["sse"][u] - r["per"][gi]))) / cv[gi])
        assert ds <= RTOL, (L, "sse", ds)
        assert dc <= RTOL, (L, "coefficients", dc)
        assert float(g["rmse"]) == float(np.sqrt(g["sse"] / dof))
        assert float(g["depth"]) == -float(g["a"]) and np.array_equal(ct["depth"][u], -ct["a"][u])
        out["sse"], out["coef"] = max(out["sse"], ds), max(out["coef"], dc)
    assert out["ties"] <= TIE_SHARE * max(1, out["reaches"]), out
    return out


# ---- the recovery of docs/channels.md, "One width per reach" ------------------------------------------------------------------
# channel_reference.recovery_case's surface and cells as ONE reach; the noise was raised from 0.05 in the steps below, and
# REC_NOISE is the first of them at which the single-cell restatement finds the true index in fewer than half the cells
REC_STEPS = (0.3, 0.4, 0.5)
REC_NOISE = REC_STEPS[-1]
# ... as the restatement measures it (tests/test_channel_segments_host.py): the cells, of 100, in which the single-cell fit
# finds the true index at each step
REC_HITS = (73, 64, 49)


def recovery(noise=None, D=None):
    """The recovery case as a case dict at the given noise (REC_NOISE) and shift range (the recovery's 8)."""
    noise = REC_NOISE if noise is None else noise
    z, cells, theta, _ = cr.recovery_case(noise)
    D = cr.REC["D"] if D is None else D
    return dict(name="reach recovery noise %g D %d" % (noise, D), z=z, de=1.0, cells=np.ascontiguousarray(cells, dtype=np.int64),
                labels=np.ones(len(cells), dtype=np.int64), angle=np.full(len(cells), theta), h=cr.REC["h"], w=cr.REC["w"], D=D,
                frequencies=cr.REC["frequencies"], delta=1.0, min_samples=4, min_profiles=1)


def single_cell_hits(case):
    """In how many of the case's cells the single-cell restatement (channel_reference.choose_cell on the shared stage one)
    finds the true frequency."""
    rows = [cr.choose_cell(c, case["de"], case["D"], case["frequencies"], case["delta"]) for c in stage_of(case)]
    return sum(1 for r in rows if r["f_index"] == cr.REC["index"])


# ---- the inputs of tests/test_gpu_channel_segments.py -----------------------------------------------------------------------------
_CASES = None


def gpu_cases():
    """The cases as dicts: name, z, de, cells (int64), labels (one per cell), angle (one per cell), h, w, D, frequencies,
    delta, min_samples, min_profiles.  Every case runs in both modes.  DEMs are 96 x 128 but for the 64 frequencies at h = 100
    (256 x 256).  Seeded: the same on every box."""
    global _CASES
    if _CASES is not None:
        return _CASES
    cases = []

    def add(name, z, de, cells, labels, angle, h, w, D, freqs, delta=1.0, ms=4, mp=1):
        cells = np.ascontiguousarray(cells, dtype=np.int64)
        angle = np.ascontiguousarray(np.broadcast_to(np.asarray(angle, dtype=np.float64), cells.shape))
        cases.append(dict(name=name, z=z, de=float(de), cells=cells, labels=np.asarray(labels, dtype=np.int64), angle=angle, h=h,
                          w=w, D=D, frequencies=np.ascontiguousarray(freqs, dtype=np.float64), delta=delta, min_samples=ms,
                          min_profiles=mp))

    rng = np.random.default_rng(20261021)
    f0 = float(cr.freqs_of_sigma([4.0])[0])
    zs = cr.channel_z(128, ny=96, f0=f0)                                    # the trough of the small cases: 4 cells wide
    ny, nx = zs.shape

    def line(k, lo=14, hi=82, off=3):
        return cr.line_cells(128, 96, rng.integers(lo, hi, k)) + rng.integers(-off, off + 1, k)

    # reaches of 1, 2, 63, 64, 65 and 129 usable profiles in one call - both sides of the 64-profile block of the sum and three
    # blocks -, labels <= 0 mixed in, the cells in shuffled order; short profiles (h = 8)
    sizes = [1, 2, 63, 64, 65, 129]
    lab = np.concatenate([np.repeat([7, 2, 9, 4, 11, 5], sizes), [0, -3, 0, -1, 0, 0]])
    perm = rng.permutation(len(lab))
    add("sizes 1 2 63 64 65 129, h = 8, labels <= 0", zs, 1.0, line(len(lab))[perm], lab[perm],
        (0.2 + 0.05 * rng.standard_normal(len(lab)))[perm], 8, 1, 2, cr.freqs_of_sigma(np.geomspace(1.0, 6.0, 6)))
    # a reach with unusable cells in the middle (cells on the left edge at orientation 0 have nothing at j < 0), one with no
    # usable cell, one below min_profiles; and one with dof < 1: min_samples is 2 and a row of the DEM is NaN but for what
    # leaves its cell the four points j = -3, -2, 1, 2 (a sample reads its right-hand neighbour, with weight 0)
    zh = zs.copy()
    zh[88, :] = np.nan
    zh[88, 57:60] = zs[88, 57:60]
    zh[88, 61:64] = zs[88, 61:64]
    good = line(12, 20, 70)
    left = rng.integers(20, 70, 5) * nx
    cells = np.concatenate([good[:4], left[:3], good[4:7], left[3:], good[7:9], [88 * nx + 60], good[9:]])
    lab = np.concatenate([np.full(10, 3), np.full(2, 1), np.full(2, 8), [6], np.full(3, 4)])
    ang = np.concatenate([0.2 + 0.05 * rng.standard_normal(4), np.zeros(3), 0.2 + 0.05 * rng.standard_normal(3), np.zeros(2),
                          np.full(2, 0.2), [0.0], np.full(3, 0.2)])
    add("unusable cells, none usable, min_profiles 3, dof < 1", zh, 1.0, cells, lab, ang, 20, 0, 3,
        cr.freqs_of_sigma(np.geomspace(0.8, 10.0, 12)), ms=2, mp=3)
    on = line(36, 30, 66)
    ang = 0.2 + 0.05 * rng.standard_normal(36)
    lab3 = rng.integers(1, 4, 36)
    add("F = 1", zs, 1.0, on[:20], lab3[:20], ang[:20], 20, 2, 3, [f0])
    add("F = 35, D = 8", zs, 1.0, on[:24], lab3[:24], ang[:24], 40, 2, 8, cr.freqs_of_sigma(np.geomspace(0.5, 20.0, 35)))
    zb = cr.channel_z(256, f0=float(cr.freqs_of_sigma([6.0])[0]))
    mid = cr.line_cells(256, 256, np.arange(110, 146, 3)) + rng.integers(-3, 4, 12)
    add("F = 64, h = 100, D = 8", zb, 1.0, mid, np.repeat([2, 1], [7, 5]), 0.2, 100, 1, 8,
        cr.freqs_of_sigma(np.geomspace(0.5, 50.0, 64)))
    add("D = 0", zs, 1.0, on, lab3, ang, 30, 2, 0, cr.freqs_of_sigma(np.geomspace(0.5, 15.0, 12)))
    add("D = h - min_samples", zs, 1.0, on[:20], lab3[:20], ang[:20], 12, 1, 8, cr.freqs_of_sigma(np.geomspace(0.7, 6.0, 10)))
    add("de = 2", zs, 2.0, on, lab3, ang, 30, 5, 4, cr.freqs_of_sigma(2.0 * np.geomspace(1.0, 14.0, 12)), delta=2.0)
    # NaN cells: scattered holes, so that a reach holds complete and incomplete profiles - both routes of the search in one sum
    zn = zs.copy()
    zn[rng.random(zn.shape) < 0.004] = np.nan
    add("NaN cells", zn, 1.0, line(40, 24, 72), rng.integers(1, 4, 40), 0.2 + 0.05 * rng.standard_normal(40), 20, 0, 3,
        cr.freqs_of_sigma(np.geomspace(0.5, 10.0, 12)), ms=6)
    # a hole at the centre at pi f de = 6: the narrowest trough is one entry of 1 and, four points out, 1e-250.  A hole over
    # j = -3..3 of ONE profile of reach 1 leaves that frequency dead in it, and so in the reach; reach 2 keeps it
    zd = zs.copy()
    zd[40, 57:64] = np.nan
    hole = np.array([44 * nx + 60, 40 * nx + 60, 48 * nx + 61, 52 * nx + 61, 56 * nx + 62, 60 * nx + 62])
    add("a hole at the centre at pi f de = 6", zd, 1.0, hole, [1, 1, 1, 2, 2, 2], 0.0, 20, 0, 0,
        np.concatenate([cr.freqs_of_sigma(np.geomspace(1.0, 8.0, 7)), [6.0 / np.pi]]))
    add("every frequency dead", zd, 1.0, hole[:4], [1, 1, 2, 2], 0.0, 20, 0, 0, [6.0 / np.pi])
    _CASES = cases
    return cases
