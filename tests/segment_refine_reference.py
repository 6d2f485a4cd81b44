"""numpy restatement of sc_fit_segments_refine (docs/segments.md, "Continuous ages"; include/scarplet_hip.h): the grid fit of
tests/segment_reference.py, then the brackets, the candidates and the picks of the definition written out on the segment's
POOLED sse - ``segment_reference.fit_age`` (ONE float64 ``lstsq`` on the full design matrix) per candidate, or
``fit_age_longdouble`` (per-profile orthogonalisation in np.longdouble) for the second arithmetic - and the rule by which a
set of tables is compared with it.  The rules of the minimum and of the interval are those of tests/refine_reference.py with
the segment's pooled grid curve for the cell's and the segment's dof for n - 3."""
import numpy as np
from scipy.special import erf

import profile_reference as pr
import refine_reference as rf
import segment_reference as sg

RTOL, COND_MAX, TIE_SHARE = pr.RTOL, pr.COND_MAX, pr.TIE_SHARE
MARGIN_MIN = 1e-8                 # below it two implementations that are each within RTOL may part
FINE_FLOATS = ("kt_fine", "kt_lo_fine", "kt_hi_fine", "a_fine", "sse_fine", "rmse_fine", "height_fine")
CELL_FLOATS = ("b_fine", "c0_fine", "sse_fine")
LEVELS = (1, 2)
candidates = rf.candidates


def fit_age_longdouble(svals, pvals, kt):
    """segment_reference.fit_age's answer by the per-profile orthogonalisation in np.longdouble (the erf column itself is
    scipy's float64): (coefficients, sse, per-profile sse, 0.0)."""
    L = np.longdouble
    terms, See, Sep = [], L(0), L(0)
    for s, p in zip(svals, pvals):
        e = erf(s / (2 * np.sqrt(kt))).astype(L)
        s, p = s.astype(L), p.astype(L)
        n = L(len(s))
        sbar, pbar, ebar = s.sum() / n, p.sum() / n, e.sum() / n
        sc = s - sbar
        sss = (sc * sc).sum()
        beta, gamma = (sc * (p - pbar)).sum() / sss, (sc * (e - ebar)).sum() / sss
        e2, p2 = (e - ebar) - gamma * sc, (p - pbar) - beta * sc
        See, Sep = See + (e2 * e2).sum(), Sep + (e2 * p2).sum()
        terms.append((s, p, e, sbar, pbar, ebar, beta, gamma))
    a = Sep / See
    coef, per = [], []
    for s, p, e, sbar, pbar, ebar, beta, gamma in terms:
        b = beta - a * gamma
        c0 = pbar - a * ebar - b * sbar
        res = p - (c0 + b * s + a * e)
        coef += [c0, b]
        per.append((res * res).sum())
    return np.array(coef + [a], dtype=L), np.sum(np.array(per, dtype=L)), np.array(per, dtype=L), 0.0


def profiles_of(case, pos):
    """(svals, pvals, used) of the cells at input positions ``pos``: the valid points of every usable profile, in order."""
    z, h, w, de = case["z"], case["h"], case["w"], case["de"]
    j = np.arange(-h, h + 1)
    svals, pvals, used = [], [], []
    for k in pos:
        r, c = divmod(int(case["cells"][k]), z.shape[1])
        p = pr.sample_profile(z, float(r), float(c), np.sin(case["angle"][k]), np.cos(case["angle"][k]), h, w)
        ok = ~np.isnan(p)
        u = int((ok & (j < 0)).sum()) >= case["min_samples"] and int((ok & (j > 0)).sum()) >= case["min_samples"]
        used.append(u)
        if u:
            svals.append((j.astype(np.float64) * de)[ok])
            pvals.append(p[ok])
    return svals, pvals, np.array(used, dtype=bool)


def grid_row(svals, pvals, n_cells, ages, delta, min_profiles, fit):
    """The grid fit of one segment in the arithmetic ``fit``: segment_reference.fit_segment's row, with 'fits' (per age)."""
    m, n = len(svals), int(sum(len(s) for s in svals))
    row = {"n_cells": n_cells, "n_profiles": m, "n": n, "dof": n - 2 * m - 1, "kt_index": -1, "lo_index": -1, "hi_index": -1,
           "status": 1, "curve": np.full(len(ages), np.nan), "cond": 0.0, "ptp": np.nan}
    for f in sg.ROW_FLOATS:
        row[f] = np.nan
    if m < min_profiles or row["dof"] < 1:
        return row
    fits = [fit(svals, pvals, kt) for kt in ages]
    sse = np.array([float(f[1]) for f in fits])
    best, lo, hi, status = pr.choose(sse, row["dof"] + 3, delta)
    row.update(kt_index=best, lo_index=lo, hi_index=hi, status=status, kt=float(ages[best]), kt_lo=float(ages[lo]),
               kt_hi=float(ages[hi]), a=float(fits[best][0][-1]), sse=float(sse[best]), rmse=float(np.sqrt(sse[best] / row["dof"])),
               curve=sse, fits=fits, cond=max(f[3] for f in fits), ptp=max(float(p.max() - p.min()) for p in pvals))
    return row


def refine_segment(row, svals, pvals, ages, R, delta, fit=sg.fit_age):
    """The fine fields of one fitted segment as a dict: refine_reference.refine_cell on the pooled criterion.  Besides the
    fields: 'coef' and 'per' (the joint fit at kt_fine: (c0_0, b_0, ..., a) and each usable profile's sse), 'margin' (for the
    minimum, the lower and the upper end: how close the nearest decision on the way came to going the other way, relative)
    and 'cond' (the largest condition number of a candidate's design matrix)."""
    A, dof, i = len(ages), row["dof"], row["kt_index"]
    curve = np.asarray(row["curve"], dtype=np.float64)
    conds = [0.0]

    def fits(x):
        out = [fit(svals, pvals, v) for v in x]
        conds.append(max(f[3] for f in out))
        return out, np.array([float(f[1]) for f in out])

    best = dict(x=float(ages[i]), fit=row["fits"][i], sse=float(row["sse"]))
    margin = [np.inf, np.inf, np.inf]
    lo_x, hi_x, status = float(ages[row["lo_index"]]), float(ages[row["hi_index"]]), row["status"]
    if R > 0:
        # the minimum
        pq = (ages[max(i - 1, 0)], ages[min(i + 1, A - 1)])
        for r in range(R):
            x = candidates(*pq)
            out, sse = fits(x)
            key = np.where(np.isnan(sse), np.inf, sse)
            l = int(np.argmin(key))                                        # (the first smallest)
            others = key[x != x[l]]
            if others.size:
                margin[0] = min(margin[0], float((others.min() - key[l]) / key[l]))
            pq = (x[max(l - 1, 0)], x[min(l + 1, 63)])
        if sse[l] <= best["sse"]:
            if float(x[l]) != best["x"]:
                margin[0] = min(margin[0], abs(best["sse"] - sse[l]) / best["sse"])
            best = dict(x=float(x[l]), fit=out[l], sse=float(sse[l]))
        else:
            margin[0] = min(margin[0], abs(best["sse"] - sse[l]) / best["sse"])
        thr = best["sse"] * (1.0 + delta / dof)
        status = 0
        # the lower end
        g = int(np.flatnonzero(ages <= best["x"]).max())
        j = g
        while j >= 0 and curve[j] <= thr:
            j -= 1
        margin[1] = rf._gap(curve[max(j, 0):g + 1], thr)
        if j < 0:
            lo_x, status = float(ages[0]), status | 2
        else:
            pq = (ages[j], ages[j + 1] if j + 1 <= g else best["x"])
            for r in range(R):
                x = candidates(*pq)
                _, sse = fits(x)
                ok = sse <= thr
                ok[63] = True
                l = 1 + int(np.argmax(ok[1:]))
                margin[1] = min(margin[1], rf._gap(sse[1:63], thr))
                pq = (x[l - 1], x[l])
            lo_x = float(pq[1])
        # the upper end
        g = int(np.flatnonzero(ages >= best["x"]).min())
        j = g
        while j <= A - 1 and curve[j] <= thr:
            j += 1
        margin[2] = rf._gap(curve[g:min(j, A - 1) + 1], thr)
        if j > A - 1:
            hi_x, status = float(ages[A - 1]), status | 4
        else:
            pq = (ages[j - 1] if j - 1 >= g else best["x"], ages[j])
            for r in range(R):
                x = candidates(*pq)
                _, sse = fits(x)
                ok = sse <= thr
                ok[0] = True
                l = 62 - int(np.argmax(ok[:63][::-1]))
                margin[2] = min(margin[2], rf._gap(sse[1:63], thr))
                pq = (x[l], x[l + 1])
            hi_x = float(pq[0])
    coef = np.array([float(v) for v in best["fit"][0]])
    a = float(coef[-1])
    return dict(kt_fine=best["x"], kt_lo_fine=lo_x, kt_hi_fine=hi_x, a_fine=a, sse_fine=best["sse"],
                rmse_fine=float(np.sqrt(best["sse"] / dof)), height_fine=2.0 * a, status_fine=int(status), margin=margin,
                coef=coef, per=np.array([float(v) for v in best["fit"][2]]), cond=max(conds))


def restate(case, R, fit=sg.fit_age):
    """The rows of a case at R levels, one per distinct positive label in ascending order: grid_row's fields, 'label',
    'where' (the input positions of the segment's cells), 'used' (one bool per cell), the fine fields, 'cells' (b_fine,
    c0_fine, sse_fine per cell of the segment, NaN where the profile is not used or the segment not fitted) and, where the
    segment is fitted, 'svals' and 'pvals'."""
    ages = np.asarray(case["ages"], dtype=np.float64)
    lab, where = sg.group(case["labels"])
    rows = []
    for L, pos in zip(lab, where):
        svals, pvals, used = profiles_of(case, pos)
        row = grid_row(svals, pvals, len(pos), ages, case["delta"], case["min_profiles"], fit)
        row.update(label=int(L), where=pos, used=used)
        cells = {f: np.full(len(pos), np.nan) for f in CELL_FLOATS}
        if row["status"] == 1:
            row.update({f: np.nan for f in FINE_FLOATS}, status_fine=1, margin=[np.inf] * 3)
        else:
            fine = refine_segment(row, svals, pvals, ages, R, case["delta"], fit)
            fine["cond"] = max(fine["cond"], row["cond"])
            row.update(fine, svals=svals, pvals=pvals)
            cells["c0_fine"][used], cells["b_fine"][used] = fine["coef"][0:-1:2], fine["coef"][1:-1:2]
            cells["sse_fine"][used] = fine["per"]
        row["cells"] = cells
        rows.append(row)
    return rows


def device_rows(table, cell_table, ref):
    """The device's tables in the shape compare takes: per segment the row's fields and 'cells' - the fine fields of the cell
    table (in input order of the kept cells, indexed by input position) at the segment's cells."""
    out = []
    for g, r in zip(table, ref):
        d = {f: g[f] for f in table.dtype.names}
        d["cells"] = {f: np.asarray(cell_table[f][r["where"]], dtype=np.float64) for f in CELL_FLOATS}
        out.append(d)
    return out


def compare(ref, got, case, R):
    """``got`` (per segment, anything indexable by the fine fields' names, n_profiles, dof, status, sse and 'cells') against
    ``ref`` (restate's rows in float64 lstsq).  Asserts what is exact or within RTOL, and returns the figures: segments,
    fitted, ties (segments where a pick parted that the restatement had decided within RTOL), the largest relative sse
    difference, the largest coefficient difference over the profiles' range, the largest condition number, the smallest
    margin."""
    h, de = case["h"], case["de"]
    ages = np.asarray(case["ages"], dtype=np.float64)
    out = {"segments": len(ref), "fitted": 0, "ties": 0, "sse": 0.0, "coef": 0.0, "cond": 0.0, "margin": np.inf}
    assert len(got) == len(ref)
    for r, g in zip(ref, got):
        L = r["label"]
        assert int(g["n_profiles"]) == r["n_profiles"] and int(g["dof"]) == r["dof"], L
        assert (int(g["status"]) & 1) == (r["status"] & 1), L
        gc = g["cells"]
        if r["status"] == 1:
            assert int(g["status_fine"]) == 1 and all(np.isnan(float(g[f])) for f in FINE_FLOATS), L
            assert all(np.isnan(gc[f]).all() for f in CELL_FLOATS), L
            continue
        out["fitted"] += 1
        assert r["cond"] <= COND_MAX, ("the inputs leave the tolerance's ground", L, r["cond"])
        out["cond"], out["margin"] = max(out["cond"], r["cond"]), min(out["margin"], min(r["margin"]))
        fine = {f: float(g[f]) for f in FINE_FLOATS}
        dof, u = r["dof"], r["used"]
        # structure: what the definition gives whatever was picked
        assert fine["kt_lo_fine"] <= fine["kt_fine"] <= fine["kt_hi_fine"], L
        assert ages[0] <= fine["kt_lo_fine"] and fine["kt_hi_fine"] <= ages[-1], L
        assert fine["sse_fine"] <= float(g["sse"]), L
        assert fine["rmse_fine"] == float(np.sqrt(np.float64(fine["sse_fine"]) / dof)), L
        assert fine["height_fine"] == 2.0 * fine["a_fine"], L
        assert all(np.isnan(gc[f][~u]).all() and not np.isnan(gc[f][u]).any() for f in CELL_FLOATS), L
        # sse_fine and the coefficients against float64 lstsq at the age that was picked, unconditionally
        coef, sse, per, cond = sg.fit_age(r["svals"], r["pvals"], fine["kt_fine"])
        assert cond <= COND_MAX, L
        ds = max(abs(fine["sse_fine"] - sse) / sse, float(np.max(np.abs(gc["sse_fine"][u] - per))) / sse)
        dc = max(abs(fine["a_fine"] - coef[-1]), float(np.max(np.abs(gc["c0_fine"][u] - coef[0:-1:2]))),
                 float(np.max(np.abs(gc["b_fine"][u] - coef[1:-1:2]))) * h * de) / r["ptp"]
        assert ds <= RTOL, (L, "sse_fine", ds)
        assert dc <= RTOL, (L, "coefficients", dc)
        out["sse"], out["coef"] = max(out["sse"], ds), max(out["coef"], dc)
        # the picks: bit-equal, or parted where the restatement's own decision lay within RTOL
        tie = False
        if fine["kt_fine"] != r["kt_fine"]:
            assert r["margin"][0] <= RTOL, (L, "kt_fine", fine["kt_fine"], r["kt_fine"], r["margin"])
            tie = True
        else:
            for e, f in ((1, "kt_lo_fine"), (2, "kt_hi_fine")):
                if fine[f] != r[f]:
                    assert r["margin"][e] <= RTOL, (L, f, fine[f], r[f], r["margin"])
                    tie = True
        if tie:
            out["ties"] += 1
        else:
            assert int(g["status_fine"]) == r["status_fine"], (L, g["status_fine"], r["status_fine"])
    assert out["ties"] <= TIE_SHARE * max(1, out["segments"]), out
    return out


def close_margins(ref):
    """The segments of restate's rows with any margin below MARGIN_MIN."""
    return sum(1 for r in ref if r["status"] != 1 and min(r["margin"]) < MARGIN_MIN)


# ---- the inputs of tests/test_gpu_segment_refine.py (and of the two-arithmetics test on the CPU) -------------------------------
NAMES = ["synthetic", "sizes 1 2 64 65 130", "one age", "64 ages", "best age below the grid", "best age above the grid",
         "min_profiles 25", "unusable segment", "no cell", "labels <= 0 only", "NaN cells and borders", "shuffled order",
         "repeated cells", "120 segments of 3", "h1024"]

SEED = 20261021
QUIET = 0.005                     # the noise of the cases' own surfaces
ALIGNED = 1e-4                    # ... and of the surface whose scarp runs along a column
_CASES = []


def build_cases(seed):
    """The cases for one seed.  The cells lie ON the scarp's line (refine_reference.line_cells) wherever the case leaves their
    place free: off it the pooled sse is the misfit of a step that is not centred, its curve is flat, and the picks of the
    second level - candidates 1e-4 apart in kt - are decided inside 1e-8.  The seed is chosen so that every decision of the
    restatement keeps a margin of 1e-8 (tests/test_segment_refine_host.py).  For the same reason the surface is QUIET, noise 0.005
    for segment_reference's 0.05: the curvature of the pooled sse about its minimum, relative to the minimum, goes with the
    inverse square of the noise, and with it every margin of the last level - with delta = 0 an end is searched right beside the
    minimum, where at noise 0.05 the candidates lie within 1e-8 of thr by construction."""
    from scarplet_amd import _plan
    ages = _plan.age_grid()
    theirs = {c["name"]: c for c in sg.gpu_cases()}
    fine = {c["name"]: c for c in rf.gpu_cases()}
    rng = np.random.default_rng(seed)
    cases = []

    def add(name, z, de, cells, labels, angle, h, w, kt=ages, delta=1.0, ms=4, mp=1):
        cells = np.ascontiguousarray(cells, dtype=np.int64)
        angle = np.ascontiguousarray(np.broadcast_to(np.asarray(angle, dtype=np.float64), cells.shape))
        cases.append(dict(name=name, z=z, de=float(de), cells=cells, labels=np.asarray(labels, dtype=np.int64), angle=angle,
                          h=h, w=w, ages=np.asarray(kt, dtype=np.float64), delta=delta, min_samples=ms, min_profiles=mp))

    def on_line(k):
        return rf.line_cells(600, 0.2, rng.integers(150, 450, k))

    # segment_reference's eight interleaved segments of 120 cells - its labels and spread of orientations - at w = 2
    t = theirs["synthetic h100 w5"]
    z = pr.synthetic_z(600, sigma=QUIET)
    add("synthetic", z, 1.0, on_line(120), t["labels"], 0.2 + 0.05 * rng.standard_normal(120), 100, 2, ms=15)
    # one profile, both sides of the 64-profile block of the segmented sum, and three blocks (the restatement's matrix is
    # rebuilt for every candidate: 130 profiles, not 2100)
    sizes = [1, 2, 64, 65, 130]
    lab = np.repeat([5, 1, 9, 2, 7], sizes)
    add("sizes 1 2 64 65 130", z, 1.0, on_line(len(lab)), lab, 0.2 + 0.02 * rng.standard_normal(len(lab)), 5, 1, kt=[1.0, 3.0], ms=3)
    on = on_line(60)
    three = np.arange(60) % 3 + 1
    add("one age", z, 1.0, on, three, 0.2, 100, 2, kt=[10.0], ms=15)
    add("64 ages", z, 1.0, on, three, 0.2, 100, 2, kt=10 ** np.linspace(0, 3.4, 64), ms=15)
    # the scarp is 10 old: grids that begin above it and end below it put the minimum on their first and last age
    add("best age below the grid", z, 1.0, on, three, 0.2, 100, 2, kt=ages[14:24], ms=15)
    add("best age above the grid", z, 1.0, on, three, 0.2, 100, 2, kt=ages[:7], ms=15)
    # segments of 30, 20 and 10 profiles: one fitted, two of status 1
    add("min_profiles 25", z, 1.0, on, np.repeat([2, 1, 3], [30, 20, 10]), 0.2, 100, 2, ms=15, mp=25)
    cases.append(dict(theirs["unusable segment"]))
    cases.append(dict(theirs["no cell"]))
    cases.append(dict(theirs["labels <= 0 only"]))
    b = fine["borders, corners and NaN cells"]
    add("NaN cells and borders", b["z"], 1.0, b["cells"], np.arange(len(b["cells"])) % 4 + 1, b["angle"], b["h"], b["w"], ms=15)
    perm = rng.permutation(60)
    add("shuffled order", z, 1.0, on[perm], (np.arange(60) % 4 + 1)[perm], 0.2, 30, 2, kt=ages[:24:2], ms=10, delta=4.0)
    # delta = 0 searches either end right beside the minimum: the candidates of the last level lie within 4e-5 of kt_fine, and
    # their sse within 1e-8 of thr = sse_fine unless the curvature of the sse is some 1e2 times its minimum.  So these
    # profiles meet no misfit but the noise: the scarp runs along the middle column of an odd grid, the profiles along the
    # rows - every sample a node of the grid - and the noise is 1e-4.  The same surface serves the short profiles below
    za = pr.synthetic_z(601, theta=0.0, sigma=ALIGNED)
    rep = rf.line_cells(601, 0.0, rng.integers(150, 450, 7))
    add("repeated cells", za, 1.0, np.concatenate([np.repeat(rep, 3), rep]), np.repeat([2, 1], [21, 7]), 0.0, 100, 5,
        ms=15, delta=0.0)
    # many segments a launch; the only case with a hundred segments, where the tie cap is not zero
    add("120 segments of 3", za, 1.0, rf.line_cells(601, 0.0, rng.integers(150, 450, 360)),
        rng.permutation(np.repeat(np.arange(1, 121), 3)), 0.0, 15, 0, ms=12)
    cases[-1] = rf.cut_to_the_cap(cases[-1])
    add("h1024", pr.synthetic_z(2400, sigma=QUIET), 1.0, rf.line_cells(2400, 0.2, rng.integers(1150, 1250, 4)), np.ones(4, dtype=np.int64),
        0.2, 1024, 1, ms=100)
    assert [c["name"] for c in cases] == NAMES
    return cases


def gpu_cases():
    """The cases as dicts (segment_reference.gpu_cases's keys), by NAMES.  Seeded and built once."""
    if not _CASES:
        _CASES.extend(build_cases(SEED))
    return _CASES


_REF = {}


def reference(name, R):
    """restate() of a case in float64 lstsq, computed once and shared: not to be changed by a test."""
    if (name, R) not in _REF:
        _REF[(name, R)] = restate(gpu_cases()[NAMES.index(name)], R)
    return _REF[(name, R)]


# ---- what it recovers (docs/segments.md, "Continuous ages") -----------------------------------------------------------------
KT0 = rf.KT0
SIGMAS = (0.0, 0.05, 0.5)


def recovery_case(sigma):
    """refine_reference.recovery_case as ONE segment: the 100 cells on the line of synthetic_scarp(600, theta=0.2, kt0=KT0)
    with noise ``sigma``; h = 100, w = 2."""
    c = rf.recovery_case(sigma)
    return dict(c, labels=np.ones(len(c["cells"]), dtype=np.int64), min_profiles=1)


def recovery_figures(row):
    """(|kt / KT0 - 1|, |kt_fine / KT0 - 1|) of the one row."""
    return abs(float(row["kt"]) / KT0 - 1.0), abs(float(row["kt_fine"]) / KT0 - 1.0)
