"""numpy restatement of sc_fit_strike / sl.fit_along_strike (docs/strike.md), algebraically independent of the device's
route.  The windows are cut from the definition - a window holds the cells with ``u_k - window / 2 <= t_c <= u_k +
window / 2``, found by comparing every cell, not by a search in a sorted array - and every window's row is
``segment_reference.fit_segment`` on the window's cells in hand-over order: ONE ``np.linalg.lstsq`` on the full design
matrix per age (a dummy intercept and slope per usable profile plus the shared erf column), never the per-profile term
sums of the device and never ``SSpp - Q``.  With a centre shift it is ``shift_reference.fit_segment`` with given
``d_ci``."""
import math

import numpy as np

import bootstrap_reference as br
import profile_reference as pr
import segment_reference as sr
import shift_reference as sh

RTOL, COND_MAX, TIE_SHARE = pr.RTOL, pr.COND_MAX, pr.TIE_SHARE
SPP_MAX = 1e3        # a condition on the inputs: SSpp / sse_min of every compared window (docs/strike.md, "The subtraction")
ROW_INTS = ("label", "station", "n_cells", "n_profiles", "n", "dof")
ROW_FLOATS = ("kt", "kt_lo", "kt_hi", "a", "sse", "rmse")


def handover(cells, labels, angle, nx, de):
    """Per distinct positive label in ascending order: (label, the input positions of its cells sorted by (t, input
    position), their t, the strike).  The strike is the axial mean of the segment's angles in input order."""
    cells = np.asarray(cells, dtype=np.int64)
    lab, where = sr.group(labels)
    out = []
    for L, pos in zip(lab, where):
        a = br.strike_of(angle[pos])
        t = [de * (float(c // nx) * math.cos(a) + float(c % nx) * math.sin(a)) for c in cells[pos]]
        order = sorted(range(len(pos)), key=lambda k: (t[k], k))
        out.append((int(L), pos[order], np.array([t[k] for k in order]), a))
    return out


def stations(t, window, step):
    """(centres, [(lo, hi)]) of one segment whose cells lie at ``t`` (ascending): the definition, cell by cell."""
    tmin, span = t[0], t[-1] - t[0]
    ns = int(math.floor(span / step)) + 1
    first = tmin + (span - (ns - 1) * step) / 2
    centres, ranges = [], []
    for k in range(ns):
        u = first + k * step
        inside = [i for i in range(len(t)) if u - window / 2 <= t[i] <= u + window / 2]
        assert inside == list(range(inside[0], inside[-1] + 1)) if inside else True
        # (an empty window: the place where its cells would go)
        lo = inside[0] if inside else sum(1 for v in t if v < u - window / 2)
        centres.append(u)
        ranges.append((lo, lo + len(inside)))
    return centres, ranges


def spp_of(z, cell, sa, ca, h, w, de, min_samples):
    """The squared residuals of a usable profile about its own least-squares line (None: not usable)."""
    p, j, n, usable = sh.profile_of(z, cell, sa, ca, h, w, min_samples)
    if not usable:
        return None
    s = j.astype(np.float64) * de
    X = np.stack([np.ones_like(s), s], axis=1)
    res = p - X @ np.linalg.lstsq(X, p, rcond=None)[0]
    return float(np.sum(res * res))


def fit_along_strike(z, de, cells, labels, angle, h, w, ages, window, step, delta=1.0, min_samples=4, min_profiles=1,
                     D=0, shifts=None):
    """Rows (a list of dicts, one per (label, station) in that order): segment_reference.fit_segment's fields - or
    shift_reference.fit_segment's, with ``shifts`` (K, A) in input order, when D > 0 - plus 'label', 'station', 't',
    'row', 'col', 'where' (the input positions of the window's cells in hand-over order) and 'spp' (SSpp)."""
    z = np.asarray(z, dtype=np.float64)
    ages = np.asarray(ages, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.int64)
    angle = np.broadcast_to(np.asarray(angle, dtype=np.float64), (len(cells),))
    sa, ca = np.sin(angle), np.cos(angle)
    nx = z.shape[1]
    rows = []
    for L, pos, t, _ in handover(cells, labels, angle, nx, de):
        centres, ranges = stations(t, window, step)
        for k, (u, (lo, hi)) in enumerate(zip(centres, ranges)):
            wp = pos[lo:hi]
            if D > 0:
                row = sh.fit_segment(z, de, cells[wp], sa[wp], ca[wp], h, w, D, ages, np.asarray(shifts)[wp], delta,
                                     min_samples, min_profiles)
            else:
                row = sr.fit_segment(z, de, cells[wp], sa[wp], ca[wp], h, w, ages, delta, min_samples, min_profiles)
            spp = [spp_of(z, cells[c], sa[c], ca[c], h, w, de, min_samples) for c in wp]
            row.update(label=L, station=k, t=u, where=wp, spp=float(sum(v for v in spp if v is not None)),
                       row=float(np.mean(cells[wp] // nx)) if len(wp) else np.nan,
                       col=float(np.mean(cells[wp] % nx)) if len(wp) else np.nan)
            rows.append(row)
    return rows


def compare(ref, table, curve, ages, delta):
    """The device's table and (NW, A) curves against ``ref`` (fit_along_strike rows).  Asserts what is exact or within
    RTOL, and the conditions on the inputs; returns the figures."""
    out = {"windows": len(ref), "fitted": 0, "ties": 0, "sse": 0.0, "a": 0.0, "cond": 0.0, "spp": 0.0}
    assert len(table) == len(ref) and curve.shape == (len(ref), len(ages))
    for s, (r, g) in enumerate(zip(ref, table)):
        key = (r["label"], r["station"])
        for f in ROW_INTS:
            assert int(g[f]) == r[f], (key, f, g[f], r[f])
        assert abs(float(g["t"]) - r["t"]) <= 1e-12 * max(1.0, abs(r["t"])), (key, g["t"], r["t"])
        for f in ("row", "col"):
            assert (np.isnan(g[f]) and np.isnan(r[f])) or abs(float(g[f]) - r[f]) <= 1e-12 * max(1.0, abs(r[f])), (key, f)
        assert (int(g["status"]) & 1) == (r["status"] & 1), (key, g["status"], r["status"])
        if r["status"] == 1:
            assert int(g["status"]) == 1
            assert int(g["kt_index"]) == -1 and int(g["lo_index"]) == -1 and int(g["hi_index"]) == -1, key
            assert all(np.isnan(g[f]) for f in ROW_FLOATS) and np.isnan(g["height"]), key
            assert np.isnan(curve[s]).all(), key
            continue
        out["fitted"] += 1
        cv, dof = r["curve"], r["dof"]
        assert r["cond"] <= COND_MAX, ("the inputs leave the tolerance's ground", key, r["cond"])
        assert r["spp"] <= SPP_MAX * cv.min(), ("the inputs leave the tolerance's ground", key, r["spp"] / cv.min())
        out["cond"], out["spp"] = max(out["cond"], r["cond"]), max(out["spp"], r["spp"] / cv.min())
        gi, glo, ghi = int(g["kt_index"]), int(g["lo_index"]), int(g["hi_index"])
        tie = False
        if gi != r["kt_index"]:
            assert abs(cv[gi] - r["sse"]) <= RTOL * r["sse"], (key, gi, r["kt_index"], cv[gi], r["sse"])
            tie = True
        thr = cv[gi] * (1.0 + delta / dof)
        for gv, rv, i in ((glo, r["lo_index"], max(glo, r["lo_index"]) - 1), (ghi, r["hi_index"], min(ghi, r["hi_index"]) + 1)):
            if gv != rv:
                assert abs(cv[i] - thr) <= RTOL * thr, (key, gv, rv, cv[i], thr)
                tie = True
        assert (int(g["status"]) & 6) == (2 if glo == 0 else 0) + (4 if ghi == len(cv) - 1 else 0), (key, g["status"])
        if tie:
            out["ties"] += 1
        else:
            assert int(g["status"]) == r["status"], (key, g["status"], r["status"])
        ds = max(abs(float(g["sse"]) - cv[gi]) / cv[gi], float(np.max(np.abs(curve[s] - cv) / cv)))
        da = abs(float(g["a"]) - r["coefs"][gi][-1]) / r["ptp"]
        assert ds <= RTOL, (key, "sse", ds)
        assert da <= RTOL, (key, "a", da)
        assert float(g["sse"]) == curve[s][gi] and float(g["rmse"]) == float(np.sqrt(g["sse"] / dof)), key
        assert float(g["height"]) == 2.0 * float(g["a"]), key
        assert float(g["kt"]) == ages[gi] and float(g["kt_lo"]) == ages[glo] and float(g["kt_hi"]) == ages[ghi], key
        out["sse"], out["a"] = max(out["sse"], ds), max(out["a"], da)
    assert out["ties"] <= TIE_SHARE * max(1, out["windows"]), out
    return out


# ---- the inputs of tests/test_gpu_strike.py ---------------------------------------------------------------------------------
N = 300
# the run boundaries: (window, step) on 200 cells of one column at de = 1 (t = row) -> the count some window holds
RUNS = {1: (1.0, 1.0), 63: (62.0, 35.0), 64: (63.0, 34.0), 65: (64.0, 35.0), 128: (127.0, 34.0), 129: (128.0, 35.0),
        130: (129.0, 34.0)}


def vertical(sigma=0.3, seed=5):
    """(z, the 200 cells of rows 50..249 in the column of the scarp): synthetic_scarp(N, theta=0) - the scarp runs along
    a column, orientation 0, t = de row."""
    z = pr.synthetic_z(N, sigma=sigma, theta=0.0, seed=seed)
    x = np.linspace(-N / 2, N / 2, num=N)
    col = int(np.argmin(np.abs(x)))
    return z, np.arange(50, 250, dtype=np.int64) * N + col


def line_cells(rows, theta=0.2, off=0):
    """One cell per row of ``rows`` on the scarp's line of synthetic_scarp(N, theta) (moved ``off`` columns)."""
    x = np.linspace(-N / 2, N / 2, num=N)
    rows = np.asarray(rows, dtype=np.int64)
    yrot = -x[None, :] * np.cos(theta) + x[rows][:, None] * np.sin(theta)
    return rows * N + np.clip(np.argmin(np.abs(yrot), axis=1) + off, 0, N - 1)


def gpu_cases():
    """The cases as dicts: name, z, cells, labels, angle (one per cell), h, w (cells), ages, window, step, delta,
    min_samples, min_profiles, D - all at de = 1.  Seeded: the same on every box."""
    from scarplet_amd import _plan
    ages = _plan.age_grid()
    cases = []

    def add(name, z, cells, labels, angle, h, w, kt, window, step, delta=1.0, ms=4, mp=1, D=0):
        cells = np.ascontiguousarray(cells, dtype=np.int64)
        angle = np.ascontiguousarray(np.broadcast_to(np.asarray(angle, dtype=np.float64), cells.shape))
        cases.append(dict(name=name, z=z, cells=cells, labels=np.asarray(labels, dtype=np.int64), angle=angle, h=h, w=w,
                          ages=np.asarray(kt, dtype=np.float64), window=float(window), step=float(step), delta=delta,
                          min_samples=ms, min_profiles=mp, D=D))

    # 1. the noisy case of docs/segments.md
    z, cells, theta = sr.noisy_case()
    for window, step in ((30, 15), (60, 30), (9, 9), (400, 400)):
        add("noisy %d %d" % (window, step), z, cells, np.ones(100, dtype=int), theta, 100, 2, ages, window, step, ms=15)
    # 2. the boundaries of the runs of 64
    zv, col = vertical()
    five = [3.0, 6.0, 10.0, 18.0, 30.0]
    for count, (window, step) in RUNS.items():
        add("run %d" % count, zv, col, np.full(200, 4), 0.0, 20, 1, five, window, step)
    # 3. the lanes
    add("one age", zv, col, np.full(200, 4), 0.0, 20, 1, [10.0], 20, 10)
    add("64 ages", zv, col, np.full(200, 4), 0.0, 20, 1, 10 ** np.linspace(0, 1.6, 64), 20, 10)
    # 4. unusable profiles: rows 60 and 63 are NaN (w = 0: their cells have no profile) in the middle of a window's run,
    # rows 100..120 leave windows without a usable profile and, at their ends, with one or two; the segment has no cell
    # in rows 140..169: empty windows.  A second segment runs down the right edge, its profiles clipped to 0..7 points
    zn = zv.copy()
    zn[[60, 63], :] = np.nan
    zn[100:121, :] = np.nan
    keep = np.r_[0:90, 120:200]                                           # rows 50..139 and 170..249
    edge = np.arange(30, 70, dtype=np.int64) * N + (N - 1 - (np.arange(40) % 8))
    rng = np.random.default_rng(20261021)
    perm = rng.permutation(len(keep) + len(edge))
    un = (np.concatenate([col[keep], edge])[perm], np.repeat([3, 7], [len(keep), len(edge)])[perm], 0.0)
    add("unusable", zn, *un, 20, 0, five, 10, 5)
    add("unusable min_profiles 3", zn, *un, 20, 0, five, 10, 5, mp=3)
    # 5. several segments: strikes 0.2 (twice), a diagonal, one cell; labels not consecutive; shuffled
    zs = pr.synthetic_z(N, sigma=0.3, theta=0.2, seed=6)
    d = np.arange(100, 140, dtype=np.int64)
    parts = [line_cells(np.arange(40, 100)), d * N + d, line_cells([145]), line_cells(np.arange(150, 221))]
    lab = np.repeat([5, 2, 11, 9], [len(p) for p in parts])
    ang = np.repeat([0.2, np.pi / 4, 0.2, 0.2], [len(p) for p in parts]) + 0.02 * rng.standard_normal(len(lab))
    perm = rng.permutation(len(lab))
    add("several segments", zs, np.concatenate(parts)[perm], lab[perm], ang[perm], 20, 1, five, 12, 6)
    # 6. the centre shift: cells up to two columns off the line, D = 3
    off = rng.integers(-2, 3, 60)
    add("D 3", zs, line_cells(np.arange(60, 120)) + off, np.full(60, 8), 0.2, 20, 1, five, 16, 8, D=3)
    return cases


def restate(case, shifts=None):
    return fit_along_strike(case["z"], 1.0, case["cells"], case["labels"], case["angle"], case["h"], case["w"], case["ages"],
                            case["window"], case["step"], case["delta"], case["min_samples"], case["min_profiles"],
                            case["D"], shifts)
