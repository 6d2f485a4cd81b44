"""numpy restatement of sc_fit_segments_ramp (docs/segments.md, "The initial slope"; include/scarplet_hip.h),
algebraically independent of the device's route: per segment and (age, half-width) ONE ``np.linalg.lstsq`` in float64 on
the full fixed-effects design matrix - a dummy intercept column and a dummy slope column per usable profile plus the
shared column ``g`` formed from the table of F as the definition says, 2 n_profiles + 1 columns - handed to LAPACK
equilibrated as ``ramp_reference.fit_pair`` hands its three: every profile less its own mean (the mean goes back into its
c0), every column at unit norm.  A second restatement in ``np.longdouble`` (per-profile Gram-Schmidt, plain numpy sums
over the profiles; F, its erf and the column difference in longdouble too) is the reference-side noise floor the GPU
tolerances stand on.  The profiles are ``profile_reference.sample_profile``'s, the tables and columns
``ramp_reference``'s, the grouping ``segment_reference``'s, the walk of the interval ``profile_reference.choose``'s."""
import numpy as np

import profile_reference as pr
import ramp_reference as rr
import segment_reference as sr

RTOL, COND_MAX, TIE_SHARE = pr.RTOL, pr.COND_MAX, pr.TIE_SHARE
FREE, SLOPE = rr.FREE, rr.SLOPE
ROW_FLOATS = sr.ROW_FLOATS
ROW_INTS = ("n_cells", "n_profiles", "n")


# ---- the fits of one segment ---------------------------------------------------------------------------------------------
def profiles_of(z, cells, sa, ca, h, w, min_samples):
    """(valid j per usable profile, their p, used per cell, n per cell)."""
    jv, pv, used, cell_n = [], [], [], []
    for k, cell in enumerate(cells):
        p, j, n, usable = rr.profile_of(z, cell, sa[k], ca[k], h, w, min_samples)
        cell_n.append(n)
        used.append(int(usable))
        if usable:
            jv.append(j)
            pv.append(p)
    return jv, pv, np.array(used, dtype=np.int64), np.array(cell_n, dtype=np.int64)


def fit_pair(svals, pvals, evals):
    """One (age, half-width) of one segment: (c0 per profile, b per profile, a, per-profile sse, condition number) by one
    float64 lstsq on the full design matrix, equilibrated."""
    m, n = len(svals), sum(len(s) for s in svals)
    X = np.zeros((n, 2 * m + 1))
    y = np.empty(n)
    means = np.empty(m)
    o = 0
    for c, (s, p, e) in enumerate(zip(svals, pvals, evals)):
        means[c] = p.sum() / len(p)
        X[o:o + len(s), 2 * c] = 1.0
        X[o:o + len(s), 2 * c + 1] = s
        X[o:o + len(s), -1] = e
        y[o:o + len(s)] = p - means[c]
        o += len(s)
    norm = np.linalg.norm(X, axis=0)
    coef, _, rank, sv = np.linalg.lstsq(X / norm, y, rcond=None)
    assert rank == X.shape[1], (rank, X.shape)
    coef = coef / norm
    res = y - X @ coef
    ends = np.cumsum([len(s) for s in svals])
    per = np.array([np.sum(r * r) for r in np.split(res, ends[:-1])])
    return coef[0:-1:2] + means, coef[1:-1:2], float(coef[-1]), per, float(sv[0] / sv[-1])


def fit_all_lstsq(svals, pvals, Evals):
    """fit_pair over every pair.  Evals: per profile (A, M + 1, n_c).  Returns c0, b (A, M + 1, m), a (A, M + 1), per
    (A, M + 1, m), cond (A, M + 1)."""
    A, M1 = Evals[0].shape[:2]
    m = len(svals)
    c0, b, per = np.empty((A, M1, m)), np.empty((A, M1, m)), np.empty((A, M1, m))
    a, cond = np.empty((A, M1)), np.empty((A, M1))
    for i in range(A):
        for q in range(M1):
            c0[i, q], b[i, q], a[i, q], per[i, q], cond[i, q] = fit_pair(svals, pvals, [E[i, q] for E in Evals])
    return c0, b, a, per, cond


def fit_all_longdouble(svals, pvals, Evals):
    """The same fits in np.longdouble: every profile's column and data orthogonalised against its own (1, s), the shared
    amplitude from the pooled sums, every pair at once."""
    L = np.longdouble
    See, Sep, keep = 0, 0, []
    for s, p, E in zip(svals, pvals, Evals):
        s, p, E = s.astype(L), p.astype(L), E.astype(L)
        n = L(len(s))
        sbar, pbar, ebar = s.sum() / n, p.sum() / n, E.sum(axis=-1, keepdims=True) / n
        sc = s - sbar
        sss = (sc * sc).sum()
        beta, gamma = (sc * (p - pbar)).sum() / sss, (sc * (E - ebar)).sum(axis=-1, keepdims=True) / sss
        e2, p2 = (E - ebar) - gamma * sc, (p - pbar) - beta * sc
        See = See + (e2 * e2).sum(axis=-1)
        Sep = Sep + (e2 * p2).sum(axis=-1)
        keep.append((s, p, E, sbar, pbar, ebar[..., 0], beta, gamma[..., 0]))
    a = Sep / See
    c0, b, per = [], [], []
    for s, p, E, sbar, pbar, ebar, beta, gamma in keep:
        bc = beta - a * gamma
        cc = pbar - a * ebar - bc * sbar
        res = p - (cc[..., None] + bc[..., None] * s + a[..., None] * E)
        c0.append(cc)
        b.append(bc)
        per.append((res * res).sum(axis=-1))
    return np.stack(c0, axis=-1), np.stack(b, axis=-1), a, np.stack(per, axis=-1), None


def pairs_of_segment(z, de, cells, sa, ca, h, w, M, ages, min_samples=4, longdouble=False):
    """What does not depend on the mode, of one segment: n_cells, n_profiles, n, 'used' and 'cell_n' (one per cell) and,
    where a profile is usable, 'c0_all', 'b_all', 'per' (A x (M + 1) x n_profiles), 'a_all', 'grid' (the pooled sse_im),
    'bbar' and 'slopes' (A x (M + 1); the signed bbar + a / (m de), copysign(inf, a) at m = 0), 'cond' (the largest
    condition number; the float64 restatement alone) and 'ptp' (the largest range of a usable profile)."""
    jv, pv, used, cell_n = profiles_of(z, cells, sa, ca, h, w, min_samples)
    m, n = len(jv), int(sum(len(j) for j in jv))
    out = {"n_cells": len(cells), "n_profiles": m, "n": n, "used": used, "cell_n": cell_n, "cond": 0.0, "ptp": np.nan}
    if m == 0:
        return out
    tab, etab = rr._tables(h, M, de, ages, longdouble)
    svals = [j.astype(np.float64) * de for j in jv]
    Evals = [rr.columns(j, h, M, de, ages, tab, etab) for j in jv]
    c0, b, a, per, cond = (fit_all_longdouble if longdouble else fit_all_lstsq)(svals, pvals=pv, Evals=Evals)
    bbar = b.sum(axis=-1) / b.dtype.type(m)
    slopes = np.empty(a.shape, dtype=a.dtype)
    slopes[:, 0] = np.copysign(np.inf, a[:, 0].astype(np.float64))
    for q in range(1, M + 1):
        slopes[:, q] = bbar[:, q] + a[:, q] / a.dtype.type(q * de)
    out.update(c0_all=c0, b_all=b, a_all=a, per=per, grid=per.sum(axis=-1), bbar=bbar, slopes=slopes,
               cond=0.0 if cond is None else float(cond.max()), ptp=max(float(p.max() - p.min()) for p in pv))
    return out


def choose_segment(pairs, de, M, ages, mode=FREE, slope=None, delta=1.0, min_profiles=1):
    """One segment's row as a dict from pairs_of_segment: the fields of sc_segment_ramp_fit, plus 'keys' (A x (M + 1): what
    the choice per age compared, inf where a pair is no candidate), 'widths' (m_i) and 'curve' (sse*)."""
    A = len(ages)
    m, n = pairs["n_profiles"], pairs["n"]
    dof = n - 2 * m - 1 - (1 if mode == FREE and M > 0 else 0)
    row = dict(pairs, dof=dof, kt_index=-1, lo_index=-1, hi_index=-1, status=1, width_index=0, width=np.nan,
               initial_slope=np.nan, curve=np.full(A, np.nan), widths=np.zeros(A, dtype=np.int64))
    for f in ROW_FLOATS:
        row[f] = np.nan
    if m < min_profiles or dof < 1:
        return row
    grid = np.asarray(pairs["grid"], dtype=np.float64)
    if mode == FREE:
        keys = grid.copy()
    else:
        keys = np.abs(np.abs(np.asarray(pairs["slopes"], dtype=np.float64)) - slope)
        keys[:, 0] = np.inf
    keys[np.isnan(grid) | np.isnan(keys)] = np.inf
    pick = np.argmin(keys, axis=1)                                         # the first smallest
    curve = np.where(np.isinf(keys[np.arange(A), pick]), np.nan, grid[np.arange(A), pick])
    best, lo, hi, status = pr.choose(np.where(np.isnan(curve), np.inf, curve), dof + 3, delta)   # (choose divides by n - 3)
    q = int(pick[best])
    sse = float(curve[best])
    row.update(keys=keys, widths=pick, curve=curve, kt_index=best, lo_index=lo, hi_index=hi,
               status=status + (8 if M > 0 and q == M else 0), width_index=q, width=q * de,
               initial_slope=float(pairs["slopes"][best, q]), kt=float(ages[best]), kt_lo=float(ages[lo]),
               kt_hi=float(ages[hi]), a=float(pairs["a_all"][best, q]), sse=sse, rmse=float(np.sqrt(sse / dof)))
    return row


def pairs_of_segments(z, de, cells, labels, angle, h, w, M, ages, min_samples=4, longdouble=False):
    """pairs_of_segment of every distinct positive label in ascending order, each with 'label' and 'where' (the input
    positions of its cells, in input order)."""
    z = np.asarray(z, dtype=np.float64)
    ages = np.asarray(ages, dtype=np.float64)
    cells = np.asarray(cells)
    angle = np.broadcast_to(np.asarray(angle, dtype=np.float64), (len(cells),))
    sa, ca = np.sin(angle), np.cos(angle)
    lab, where = sr.group(labels)
    out = []
    for l, pos in zip(lab, where):
        q = pairs_of_segment(z, de, cells[pos], sa[pos], ca[pos], h, w, M, ages, min_samples, longdouble)
        q["label"], q["where"] = int(l), pos
        out.append(q)
    return out


def fit_segments(z, de, cells, labels, angle, h, w, M, ages, mode=FREE, slope=None, delta=1.0, min_samples=4,
                 min_profiles=1, pairs=None, longdouble=False):
    """Rows (a list of dicts, one per distinct positive label in ascending order); h, w and M in cells."""
    if pairs is None:
        pairs = pairs_of_segments(z, de, cells, labels, angle, h, w, M, ages, min_samples, longdouble)
    return [choose_segment(q, de, M, np.asarray(ages, dtype=np.float64), mode, slope, delta, min_profiles) for q in pairs]


# ---- comparing the device's tables with the restatement ---------------------------------------------------------------------
def compare_segments(ref, table, cell_table, curve, widths, h, de, M, mode, slope, delta):
    """The device's tables (rows in label order, the cell table indexed by input position, the (S, A) sse* curves and
    the (S, A) half-widths) against ``ref`` (choose_segment rows).  Asserts what is exact or within RTOL; returns the
    figures.  An m_i that differs from the restatement's must have been decided within RTOL by the restatement's own key -
    relative to the key with the width free (the key is an sse), to the given slope otherwise.  The curve and the indices
    are then judged at the device's m_i, on the restatement's sse.  A segment counts as a tie when an index or an m_i of it
    differs and was so decided."""
    out = {"segments": len(ref), "fitted": 0, "ties": 0, "sse": 0.0, "coef": 0.0, "cond": 0.0}
    assert len(table) == len(ref)
    for s, (r, g) in enumerate(zip(ref, table)):
        L = r["label"]
        assert int(g["label"]) == L
        for f in ROW_INTS + ("dof",):
            assert int(g[f]) == r[f], (L, f, g[f], r[f])
        ct = cell_table[r["where"]]
        assert np.array_equal(ct["used"], r["used"]) and np.array_equal(ct["n"], r["cell_n"]), L
        assert np.all(ct["label"] == L)
        assert (int(g["status"]) & 1) == (r["status"] & 1), (L, g["status"], r["status"])
        if r["status"] == 1:
            assert int(g["kt_index"]) == -1 and int(g["lo_index"]) == -1 and int(g["hi_index"]) == -1
            assert all(np.isnan(g[f]) for f in ROW_FLOATS) and np.isnan(g["height"]), L
            assert int(g["width_index"]) == 0 and np.isnan(g["width"]) and np.isnan(g["initial_slope"]), L
            assert np.isnan(curve[s]).all() and not widths[s].any()
            assert np.isnan(ct["b"]).all() and np.isnan(ct["c0"]).all() and np.isnan(ct["sse"]).all()
            continue
        out["fitted"] += 1
        assert r["cond"] <= COND_MAX, ("the inputs leave the tolerance's ground", L, r["cond"])
        out["cond"] = max(out["cond"], r["cond"])
        A = len(r["curve"])
        mi = widths[s].astype(np.int64)
        assert mi.min() >= (1 if mode == SLOPE else 0) and mi.max() <= M, (L, mi)
        tie = False
        for i in np.flatnonzero(mi != r["widths"]):
            kd, kr = r["keys"][i, mi[i]], r["keys"][i, r["widths"][i]]
            assert abs(kd - kr) <= RTOL * (slope if mode == SLOPE else kr), (L, i, mi[i], r["widths"][i], kd, kr)
            tie = True
        cv, dof = r["grid"][np.arange(A), mi], r["dof"]
        ds = float(np.max(np.abs(curve[s] - cv) / cv))
        gi, glo, ghi = int(g["kt_index"]), int(g["lo_index"]), int(g["hi_index"])
        ri = int(np.argmin(cv))
        if gi != ri:
            assert abs(cv[gi] - cv[ri]) <= RTOL * cv[ri], (L, gi, ri, cv[gi], cv[ri])
            tie = True
        rb, rlo, rhi, _ = pr.choose(cv, dof + 3, delta)
        thr = cv[gi] * (1.0 + delta / dof)
        for gv, rv, i in ((glo, rlo, max(glo, rlo) - 1), (ghi, rhi, min(ghi, rhi) + 1)):
            if gv != rv:
                assert abs(cv[i] - thr) <= RTOL * thr, (L, gv, rv, cv[i], thr)
                tie = True
        q = int(g["width_index"])
        assert q == mi[gi] and float(g["width"]) == q * de, (L, q, mi[gi])
        assert int(g["status"]) == (2 if glo == 0 else 0) + (4 if ghi == A - 1 else 0) + (8 if M > 0 and q == M else 0)
        if tie:
            out["ties"] += 1
        else:
            assert int(g["status"]) == r["status"] and q == r["width_index"] and gi == r["kt_index"], (L, g["status"])
        ds = max(ds, abs(float(g["sse"]) - cv[gi]) / cv[gi])
        assert float(g["sse"]) == curve[s][gi]
        u = r["used"] == 1
        assert np.isnan(ct["b"][~u]).all() and np.isnan(ct["c0"][~u]).all() and np.isnan(ct["sse"][~u]).all(), L
        dc = max(abs(float(g["a"]) - r["a_all"][gi, q]), float(np.max(np.abs(ct["c0"][u] - r["c0_all"][gi, q]))),
                 float(np.max(np.abs(ct["b"][u] - r["b_all"][gi, q]))) * h * de) / r["ptp"]
        # each profile's share of the pooled sum, against the pooled sum
        ds = max(ds, float(np.max(np.abs(ct["sse"][u] - r["per"][gi, q]))) / cv[gi])
        assert ds <= RTOL, (L, "sse", ds)
        assert dc <= RTOL, (L, "coefficients", dc)
        # the initial slope is that of the row's own a and of the cell table's mean b, to the rounding of the mean
        ga = float(g["a"])
        if q == 0:
            assert float(g["initial_slope"]) == np.copysign(np.inf, ga), (L, g["initial_slope"])
        else:
            # (a sum of at most a few hundred b_c in another order: a few hundred roundings of the largest term, 1e-13)
            bm = float(np.mean(ct["b"][u]))
            want = bm + ga / (q * de)
            assert abs(float(g["initial_slope"]) - want) <= 1e-12 * max(float(np.max(np.abs(ct["b"][u]))), abs(ga) / (q * de)), \
                (L, g["initial_slope"], want)
            assert abs(float(g["initial_slope"]) - float(r["slopes"][gi, q])) * h * de <= RTOL * r["ptp"] * (1 + h / q), L
        assert float(g["rmse"]) == float(np.sqrt(g["sse"] / dof)) and float(g["height"]) == 2.0 * ga
        out["sse"], out["coef"] = max(out["sse"], ds), max(out["coef"], dc)
    assert out["ties"] <= TIE_SHARE * max(1, out["segments"]), out
    return out


# ---- the inputs of tests/test_gpu_segment_ramp.py (and of the restatements' agreement on the CPU) ---------------------------
# how far each case's age grid goes (the number of default ages, or the exponent of the last of the 64): chosen on the CPU
# so that no compared (age, half-width) passes COND_MAX and the float64 restatement and its longdouble twin agree within
# RTOL / 100 in every sse and coefficient, with no index and no m_i decided differently (tests/test_segment_ramp_host.py)
NA = {"h100 w0 M8": 35, "h30 w5 M4": 32, "sizes 1 2 64 65 130": 2, "M = h - min_samples": 25, "64 ages M1": 3.4, "de 2": 35,
      "repeated cells": 35, "borders": 35, "unusable segment": 35, "NaN cells": 33, "min_profiles 5": 35}
NAMES = ["h100 w0 M8", "h30 w5 M4", "sizes 1 2 64 65 130", "M = h - min_samples", "one age M8", "64 ages M1", "de 2",
         "repeated cells", "no cell", "labels <= 0 only", "borders", "unusable segment", "NaN cells", "min_profiles 5",
         "dof < 1 with the width free"]


def gpu_cases():
    """The cases as dicts: name, z, de, cells, labels, angle, h, w, M, ages, delta, min_samples, min_profiles, slope (the
    given slope of the run in that mode).  The surfaces and cells are those of ramp_reference.gpu_cases() wherever it has
    the case.  Seeded: the same on every box."""
    from scarplet_amd import _plan
    ages = _plan.age_grid()
    by = {c["name"]: c for c in rr.gpu_cases()}
    cases = []

    def add(name, z, de, cells, labels, angle, h, w, M, kt, slope=0.3, delta=1.0, ms=4, mp=1):
        cells = np.ascontiguousarray(cells, dtype=np.int64)
        angle = np.ascontiguousarray(np.broadcast_to(np.asarray(angle, dtype=np.float64), cells.shape))
        cases.append(dict(name=name, z=z, de=float(de), cells=cells, labels=np.asarray(labels, dtype=np.int64), angle=angle,
                          h=h, w=w, M=M, ages=np.asarray(kt, dtype=np.float64), delta=delta, min_samples=ms, min_profiles=mp,
                          slope=slope))

    rng = np.random.default_rng(20261021)
    c = by["h100 w0 M8"]
    z, on, ang = c["z"], c["cells"], c["angle"]
    lab = rng.integers(1, 9, len(on)) * 3                                  # eight segments, their cells interleaved
    add("h100 w0 M8", z, 1.0, on, lab, ang, 100, 0, 8, ages[:NA["h100 w0 M8"]], ms=15)
    add("h30 w5 M4", z, 1.0, on, lab, ang, 30, 5, 4, ages[:NA["h30 w5 M4"]], ms=15)
    # segments of 1, 2, 64, 65 and 130 usable profiles in one call: both sides of the 64-profile block of the segmented sum,
    # and a third block.  Short profiles and two young ages
    sizes = [1, 2, 64, 65, 130]
    lab = np.repeat([5, 1, 9, 2, 7], sizes)
    big = pr.scarp_cells(600, len(lab), rng, spread=1.0)
    add("sizes 1 2 64 65 130", z, 1.0, big, lab, 0.2 + 0.02 * rng.standard_normal(len(lab)), 12, 1, 2, [1.0, 3.0], ms=4)
    c = by["M = h - min_samples"]
    add("M = h - min_samples", z, 1.0, c["cells"], np.arange(len(c["cells"])) % 3 + 1, 0.2, 12, 1, 8,
        ages[:NA["M = h - min_samples"]], ms=4)
    add("one age M8", z, 1.0, on[:30], np.arange(30) % 3 + 1, 0.2, 100, 2, 8, [10.0], ms=15)
    # 203 rows of 64 ages are 104 KB: the table of F in global memory; 128 columns, two chunks of the sums
    add("64 ages M1", z, 1.0, on[:12], np.arange(12) % 2 + 1, 0.2, 100, 2, 1, 10 ** np.linspace(0, NA["64 ages M1"], 64),
        slope=0.9, ms=15)
    c = by["de 2"]
    add("de 2", c["z"], 2.0, c["cells"], np.arange(len(c["cells"])) % 4 + 2, c["angle"], 50, 2, 6, ages[:NA["de 2"]], slope=0.15,
        ms=10)
    add("repeated cells", z, 1.0, np.concatenate([np.repeat(on[:5], 3), on[:5]]), np.repeat([2, 1], [15, 5]), 0.2, 100, 5, 4,
        ages[:NA["repeated cells"]], ms=15, delta=0.0)
    add("no cell", z, 1.0, on[:0], on[:0], 0.2, 100, 5, 8, ages, ms=15)
    add("labels <= 0 only", z, 1.0, on[:5], [0, -1, 0, 0, -7], 0.2, 100, 5, 8, ages, ms=15)
    c = by["borders and corners"]
    n = c["z"].shape[0]
    add("borders", c["z"], 1.0, c["cells"], rng.integers(1, 6, len(c["cells"])), c["angle"], 100, 5, 3, ages[:NA["borders"]], ms=20)
    # the corners at orientation 0 have nothing on one side: a segment none of whose cells is usable, next to one that is
    corners = np.array([0, n - 1, n * (n - 1), n * n - 1, 150 * n + 150, 151 * n + 150])
    add("unusable segment", c["z"], 1.0, corners, [4, 4, 4, 4, 6, 6], 0.0, 100, 5, 3, ages[:NA["unusable segment"]], ms=20)
    c = by["NaN cells"]
    add("NaN cells", c["z"], 1.0, c["cells"], rng.integers(1, 7, len(c["cells"])), c["angle"], 40, 3, 3, ages[:NA["NaN cells"]], ms=20)
    add("min_profiles 5", z, 1.0, on[:24], np.arange(24) % 3 + 1 + 3 * (np.arange(24) > 17), 0.2, 100, 2, 4,
        ages[:NA["min_profiles 5"]], ms=15, mp=5)
    # ramp_reference's cell of four points, a segment of its own: n = 4, one usable profile, dof = 4 - 2 - 1 - 1 = 0 with the
    # width free and 1 with the slope given; the three cells of seven points are the other segment
    c = by["dof < 1"]
    add("dof < 1 with the width free", c["z"], 1.0, c["cells"], [3, 8, 8, 8], 0.0, 3, 0, 1, [1.0, 1.5], slope=0.5, ms=2)
    assert [q["name"] for q in cases] == NAMES
    return cases


_PAIRS = {}


def case_pairs(case, longdouble=False):
    """pairs_of_segments of a case, computed once per process."""
    key = (case["name"], longdouble)
    if key not in _PAIRS:
        _PAIRS[key] = pairs_of_segments(case["z"], case["de"], case["cells"], case["labels"], case["angle"], case["h"],
                                        case["w"], case["M"], case["ages"], case["min_samples"], longdouble)
    return _PAIRS[key]


def restate(case, mode, longdouble=False):
    return [choose_segment(q, case["de"], case["M"], case["ages"], mode, case["slope"], case["delta"], case["min_profiles"])
            for q in case_pairs(case, longdouble)]


# ---- the recovery surface of docs/segments.md ------------------------------------------------------------------------------------
def recovery_rows(noise, mode, size=None, longdouble=True):
    """The rows of ramp_reference.recovery_case(noise) as one segment (size None) or cut into segments of ``size``
    consecutive cells; the given slope is ramp_reference.REC's."""
    z, cells, theta, ages = rr.recovery_case(noise)
    R = rr.REC
    labels = np.ones(len(cells), dtype=np.int64) if size is None else np.arange(len(cells)) // size + 1
    return fit_segments(z, 1.0, cells, labels, theta, R["h"], R["w"], R["M"], ages, mode, R["slope"], longdouble=longdouble)
