"""numpy restatement of sc_channel_profiles (docs/channels.md, include/scarplet_hip.h), algebraically independent of the
device's route: ``np.linalg.lstsq`` on the three equilibrated columns ``1, s, exp(-(pi f (j - d) de)^2)`` for EACH (cell,
frequency, shift) - and a second restatement of the fit alone in ``np.longdouble`` (Gram-Schmidt), the reference-side noise
floor the GPU tolerances stand on.  The profiles are ``profile_reference.sample_profile``'s, the order of the shifts
``shift_reference.shift_order``'s.  Whether a pair is dead - its See is not > 0 - is part of the definition and is decided
in float64 for both (``see64``): a longdouble See does not underflow where the float64 one does."""
import numpy as np

import profile_reference as pr
import shift_reference as sh

RTOL, COND_MAX, TIE_SHARE = pr.RTOL, pr.COND_MAX, pr.TIE_SHARE
ROW_FLOATS = ("f", "f_lo", "f_hi", "a", "b", "c0", "sse", "rmse")
DERIVED = ("depth", "sigma", "width", "width_lo", "width_hi", "area", "curvature", "centre_row", "centre_col")


def gauss_column(j, d, de, f):
    """Row j - d of the table: the Gaussian at the point j when its centre sits d cells along the profile."""
    X = (j - d).astype(np.float64) * de
    u = (np.pi * f) * X
    return np.exp(-(u * u))


def see64(s, e):
    """What is left of the column after 1 and s, squared and summed, in float64: a pair with a See that is not > 0 is dead."""
    sc = s - s.sum() / len(s)
    ec = e - e.sum() / len(s)
    e2 = ec - ((sc * ec).sum() / (sc * sc).sum()) * sc
    return float((e2 * e2).sum())


def fit_pair(s, p, e):
    """((c0, b, a), sse) of one column: float64 lstsq on the three columns, each scaled to length 1 (a narrow trough's
    column is one entry of 1 among entries down to 1e-250)."""
    X = np.stack([np.ones_like(s), s, e], axis=1)
    norm = np.linalg.norm(X, axis=0)
    coef = np.linalg.lstsq(X / norm, p, rcond=None)[0] / norm
    res = p - (coef[0] + coef[1] * s + coef[2] * e)
    return coef, float(np.sum(res * res))


def fit_pair_longdouble(s, p, e):
    """The same fit by Gram-Schmidt in np.longdouble (the column itself is numpy's float64)."""
    L = np.longdouble
    s, p, e = s.astype(L), p.astype(L), e.astype(L)
    n = L(len(s))
    sbar, pbar, ebar = s.sum() / n, p.sum() / n, e.sum() / n
    sc = s - sbar
    sss = (sc * sc).sum()
    beta, gamma = (sc * (p - pbar)).sum() / sss, (sc * (e - ebar)).sum() / sss
    e2, p2 = (e - ebar) - gamma * sc, (p - pbar) - beta * sc
    a = (e2 * p2).sum() / (e2 * e2).sum()
    b = beta - a * gamma
    c0 = pbar - a * ebar - b * sbar
    res = p - (c0 + b * s + a * e)
    return np.array([c0, b, a], dtype=L), (res * res).sum()


def conds(s, cols):
    """Condition numbers of the column-scaled design matrices (1, s, column) of the columns ``cols`` (P x n)."""
    X = np.empty((len(cols), len(s), 3))
    X[..., 0] = 1.0
    X[..., 1] = s
    X[..., 2] = cols
    X = X / np.linalg.norm(X, axis=1, keepdims=True)
    sv = np.linalg.svd(X, compute_uv=False)
    return sv[..., 0] / sv[..., -1]


def cell_pairs(z, de, cell, sa, ca, h, w, D, freqs, min_samples=4, longdouble=False):
    """Every (frequency, shift) pair of one cell as a dict: 'n', 'usable' (the min_samples rule), 'order', 'ptp', and -
    usable - 'grid' (F x ND: the sse, NaN where the pair is dead), 'coefs' (F x ND x 3: c0, b, a) and 'cond' (the largest
    condition number over the live pairs; float64 route only)."""
    order = sh.shift_order(D)
    p, j, n, usable = sh.profile_of(z, cell, sa, ca, h, w, min_samples)
    out = {"cell": int(cell), "n": n, "usable": usable, "order": order, "ptp": np.nan, "cond": 0.0}
    if not usable:
        return out
    F = len(freqs)
    s = j.astype(np.float64) * de
    dt = np.longdouble if longdouble else np.float64
    grid = np.full((F, len(order)), np.nan, dtype=dt)
    coefs = np.full((F, len(order), 3), np.nan, dtype=dt)
    live = []
    for i, f in enumerate(freqs):
        for q, d in enumerate(order):
            e = gauss_column(j, d, de, f)
            if not see64(s, e) > 0.0:
                continue
            coefs[i, q], grid[i, q] = fit_pair_longdouble(s, p, e) if longdouble else fit_pair(s, p, e)
            live.append(e)
    out.update(grid=grid, coefs=coefs, ptp=float(p.max() - p.min()))
    if live and not longdouble:
        out["cond"] = float(conds(s, np.array(live)).max())
    return out


def choose(curve, dof, delta):
    """(f_index, lo_index, hi_index, status bits 2 and 4) from one cell's sse* curve: a NaN counts as +inf and ends a walk."""
    c = np.where(np.isnan(curve), np.inf, curve)
    best = int(np.argmin(c))
    thr = c[best] * (1.0 + delta / dof)
    lo = hi = best
    while lo > 0 and c[lo - 1] <= thr:
        lo -= 1
    while hi < len(c) - 1 and c[hi + 1] <= thr:
        hi += 1
    return best, lo, hi, (2 if lo == 0 else 0) + (4 if hi == len(c) - 1 else 0)


def choose_cell(pairs, de, D, freqs, delta=1.0):
    """One cell's row from its pairs: the fields of the device's table, plus 'dof', 'curve' (sse*), 'shifts' (d_i) and what
    ``pairs`` holds."""
    F = len(freqs)
    dof = pairs["n"] - 3 - (1 if D > 0 else 0)
    row = dict(pairs, dof=dof, f_index=-1, lo_index=-1, hi_index=-1, status=1, shift_index=0, shift=np.nan,
               curve=np.full(F, np.nan), shifts=np.zeros(F, dtype=np.int64))
    for f in ROW_FLOATS:
        row[f] = np.nan
    if not pairs["usable"] or dof < 1:
        return row
    grid = pairs["grid"].astype(np.float64)
    pick = np.argmin(np.where(np.isnan(grid), np.inf, grid), axis=1)      # the first smallest in the order tried; 0 where all are dead
    curve = grid[np.arange(F), pick]
    if np.isnan(curve).all():
        row["status"] = 1 | 32
        return row
    best, lo, hi, status = choose(curve, dof, delta)
    d = int(np.array(pairs["order"])[pick[best]])
    c0, b, a = (float(v) for v in pairs["coefs"][best, pick[best]])
    sse = float(curve[best])
    row.update(curve=curve, shifts=np.array(pairs["order"])[pick], pick=pick, f_index=best, lo_index=lo, hi_index=hi,
               status=status + (8 if D > 0 and abs(d) == D else 0), shift_index=d, shift=d * de, f=float(freqs[best]),
               f_lo=float(freqs[lo]), f_hi=float(freqs[hi]), a=a, b=b, c0=c0, sse=sse, rmse=float(np.sqrt(sse / dof)))
    return row


def case_pairs(case, longdouble=False):
    sa, ca = np.sin(case["angle"]), np.cos(case["angle"])
    return [cell_pairs(case["z"], case["de"], case["cells"][k], sa[k], ca[k], case["h"], case["w"], case["D"],
                       case["frequencies"], case["min_samples"], longdouble) for k in range(len(case["cells"]))]


_ROWS = {}


def restate(case, longdouble=False, D=None):
    """The restatement's rows of a case (kept: the host tests and the device tests of one process share them)."""
    key = (case["name"], longdouble, D)
    if key not in _ROWS:
        c = case if D is None else dict(case, D=D)
        _ROWS[key] = [choose_cell(p, c["de"], c["D"], c["frequencies"], c["delta"]) for p in case_pairs(c, longdouble)]
    return _ROWS[key]


def fit_channels(z, de, cells, angle, h, w, D, freqs, delta=1.0, min_samples=4):
    z = np.asarray(z, dtype=np.float64)
    freqs = np.asarray(freqs, dtype=np.float64)
    angle = np.broadcast_to(np.asarray(angle, dtype=np.float64), (len(cells),))
    sa, ca = np.sin(angle), np.cos(angle)
    return [choose_cell(cell_pairs(z, de, cells[k], sa[k], ca[k], h, w, D, freqs, min_samples), de, D, freqs, delta)
            for k in range(len(cells))]


def derived(f, f_lo, f_hi, a):
    """depth, sigma, width, width_lo, width_hi, area, curvature from their formulas."""
    return {"depth": -a, "sigma": 1.0 / (np.sqrt(2.0) * np.pi * f), "width": 2.0 * np.sqrt(np.log(2.0)) / (np.pi * f),
            "width_lo": 2.0 * np.sqrt(np.log(2.0)) / (np.pi * f_hi), "width_hi": 2.0 * np.sqrt(np.log(2.0)) / (np.pi * f_lo),
            "area": -a / (np.sqrt(np.pi) * f), "curvature": -2.0 * (np.pi * f) ** 2 * a}


# ---- comparing the device's table with the restatement ---------------------------------------------------------------------
def rel(x, y):
    return abs(x - y) / y


def compare_rows(ref, table, curve, shifts, h, de, D, delta):
    """The device's table, (K, F) sse* curves and (K, F) shifts against ``ref`` (choose_cell rows): the rules of
    shift_reference.compare_rows.  Asserts what is exact or within RTOL; returns the figures.  A cell counts as a tie when
    an index or a shift of it differs from the restatement's and was decided within RTOL by the restatement's own sse."""
    out = {"cells": len(ref), "fitted": 0, "ties": 0, "sse": 0.0, "coef": 0.0, "cond": 0.0, "dead": 0}
    for k, r in enumerate(ref):
        g = table[k]
        assert int(g["n"]) == r["n"], (r["cell"], g["n"], r["n"])
        if r["status"] & 1:
            assert int(g["status"]) == r["status"], (r["cell"], g["status"], r["status"])
            assert int(g["f_index"]) == -1 and int(g["lo_index"]) == -1 and int(g["hi_index"]) == -1, r["cell"]
            assert all(np.isnan(g[f]) for f in ROW_FLOATS + DERIVED) and np.isnan(g["shift"]) and int(g["shift_index"]) == 0
            assert np.isnan(curve[k]).all() and not shifts[k].any()
            continue
        assert not int(g["status"]) & 1, (r["cell"], g["status"])
        out["fitted"] += 1
        assert r["cond"] <= COND_MAX, ("the inputs leave the tolerance's ground", r["cell"], r["cond"])
        out["cond"] = max(out["cond"], r["cond"])
        cv, dof = r["curve"], r["dof"]
        dead = np.isnan(cv)
        out["dead"] += int(dead.sum())
        assert np.array_equal(np.isnan(curve[k]), dead) and not shifts[k][dead].any(), (r["cell"], "dead frequencies")
        pos = {d: q for q, d in enumerate(r["order"])}
        tie = False
        for i in np.flatnonzero(~dead):
            d = int(shifts[k][i])
            assert d in pos, (r["cell"], i, d)
            if d != r["shifts"][i]:
                assert rel(r["grid"][i, pos[d]], cv[i]) <= RTOL, (r["cell"], i, d, r["shifts"][i], r["grid"][i, pos[d]], cv[i])
                tie = True
            assert rel(float(curve[k][i]), cv[i]) <= RTOL, (r["cell"], i, "sse*")
        gi, glo, ghi = int(g["f_index"]), int(g["lo_index"]), int(g["hi_index"])
        assert not dead[gi]
        if gi != r["f_index"]:
            assert rel(cv[gi], r["sse"]) <= RTOL, (r["cell"], gi, r["f_index"], cv[gi], r["sse"])
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
        q = pos[d]
        ds = max(rel(float(g["sse"]), r["grid"][gi, q]), rel(float(g["sse"]), float(curve[k][gi])))
        c0, b, a = r["coefs"][gi, q]
        dc = max(abs(float(g["c0"]) - c0), abs(float(g["b"]) - b) * h * de, abs(float(g["a"]) - a)) / r["ptp"]
        assert ds <= RTOL, (r["cell"], "sse", ds)
        assert dc <= RTOL, (r["cell"], "coefficients", dc)
        assert float(g["rmse"]) == float(np.sqrt(g["sse"] / dof))
        out["sse"], out["coef"] = max(out["sse"], ds), max(out["coef"], dc)
    assert out["ties"] <= TIE_SHARE * max(1, out["cells"]), out
    return out


# ---- the inputs ---------------------------------------------------------------------------------------------------------------
def freqs_of_sigma(sigma):
    """The ascending frequencies of the widths ``sigma`` (data units, any order): f = 1 / (sqrt(2) pi sigma)."""
    return np.sort(1.0 / (np.sqrt(2.0) * np.pi * np.asarray(sigma, dtype=np.float64)))


def channel_z(n, **kw):
    from scarplet_amd import synthetic
    return np.asarray(synthetic.synthetic_channel(n, **kw)._griddata, dtype=np.float64)


def line_cells(n, ny, rows, theta=0.2):
    """The cell of each row in ``rows`` at the column where |yrot| of synthetic_channel(n, ny=ny) is smallest."""
    x = np.linspace(-n / 2, n / 2, num=n)
    y = np.linspace(-ny / 2, ny / 2, num=ny)
    rows = np.asarray(rows)
    yrot = -x[None, :] * np.cos(theta) + y[rows][:, None] * np.sin(theta)
    return rows.astype(np.int64) * n + np.argmin(np.abs(yrot), axis=1)


# the recovery surface of docs/channels.md: widths of 1.5 1.12^i cells, i = 0..27, the trough's own the 14th frequency
REC = {"n": 600, "theta": 0.2, "h": 100, "w": 2, "D": 8, "index": 14, "noise": 0.05,
       "frequencies": freqs_of_sigma(1.5 * 1.12 ** np.arange(28))}


def recovery_case(noise=REC["noise"]):
    """(z, cells, theta, offsets): synthetic_channel(600, theta=0.2, f0=fs[14]) and 100 cells on its line - rows 150, 153, ...
    447 -, each moved along its row by a uniform integer offset in -6..6 (np.random.default_rng(3))."""
    n, theta = REC["n"], REC["theta"]
    z = channel_z(n, theta=theta, f0=REC["frequencies"][REC["index"]], sigma=noise)
    off = np.random.default_rng(3).integers(-6, 7, 100)
    return z, line_cells(n, n, np.arange(150, 450, 3), theta) + off, theta, off


# the search against the fit (docs/channels.md): synthetic_channel(512), its own frequency alone, orientations within 0.3 rad;
# the fit on a grid of 12 % steps around that frequency.  Compared are the cells `margin` and more from every border: there
# the search's window of half-length `scale` and the profile are complete
SEARCH = {"n": 512, "f0": 0.035, "scale": 50.0, "ang": 0.3, "h": 60, "w": 2, "D": 4, "margin": 100}
# ... as the oracle and this restatement measure it (tests/test_channels_host.py): the share of cells with amp > 0 and a < 0,
# and the median of amp / curvature
SEARCH_SHARE, SEARCH_RATIO = 1.0, 0.9856


def search_frequencies():
    return SEARCH["f0"] * 1.12 ** np.arange(-8, 9)


NAMES = ["recovery 600² h100 w2 D8 F28", "de = 2, h30 w5 D4 F12", "D = h - min_samples", "D = 0", "one frequency",
         "F = 35, D = 8", "F = 64, h = 100, D = 8", "borders and corners", "NaN cells", "repeated cells", "K = 1", "no cell",
         "no live pair"]
_CASES = None


def gpu_cases():
    """The cases of tests/test_gpu_channels.py as dicts: name, z, de, cells, angle, h, w, D, frequencies, delta,
    min_samples.  DEMs are 96 x 128 but for the recovery (600 x 600) and the 64 frequencies at h = 100 (256 x 256: a
    profile of 201 points must fit for the route of complete profiles to run).  Seeded: the same on every box."""
    global _CASES
    if _CASES is not None:
        return _CASES
    cases = []

    def add(name, z, de, cells, angle, h, w, D, freqs, delta=1.0, ms=4):
        cells = np.ascontiguousarray(cells, dtype=np.int64)
        angle = np.ascontiguousarray(np.broadcast_to(np.asarray(angle, dtype=np.float64), cells.shape))
        cases.append(dict(name=name, z=z, de=float(de), cells=cells, angle=angle, h=h, w=w, D=D,
                          frequencies=np.ascontiguousarray(freqs, dtype=np.float64), delta=delta, min_samples=ms))

    rng = np.random.default_rng(20261020)
    z, cells, theta, _ = recovery_case()
    add(NAMES[0], z, 1.0, cells, theta, REC["h"], REC["w"], REC["D"], REC["frequencies"])
    f0 = float(freqs_of_sigma([4.0])[0])
    zs = channel_z(128, ny=96, f0=f0)                                       # the trough of the small cases: 4 cells wide
    on = line_cells(128, 96, np.arange(30, 66)) + rng.integers(-3, 4, 36)   # 36 cells within 3 columns of its line
    ang = 0.2 + 0.05 * rng.standard_normal(36)
    add(NAMES[1], zs, 2.0, on, ang, 30, 5, 4, freqs_of_sigma(2.0 * np.geomspace(1.0, 14.0, 12)))
    add(NAMES[2], zs, 1.0, on[:20], ang[:20], 12, 1, 8, freqs_of_sigma(np.geomspace(0.7, 6.0, 10)))
    add(NAMES[3], zs, 1.0, on, ang, 30, 2, 0, freqs_of_sigma(np.geomspace(0.5, 15.0, 12)))
    add(NAMES[4], zs, 1.0, on[:30], 0.2, 30, 2, 3, [f0])
    add(NAMES[5], zs, 1.0, on, ang, 40, 2, 8, freqs_of_sigma(np.geomspace(0.5, 20.0, 35)))
    zb = channel_z(256, f0=float(freqs_of_sigma([6.0])[0]))
    mid = line_cells(256, 256, np.arange(110, 146, 3)) + rng.integers(-3, 4, 12)
    add(NAMES[6], zb, 1.0, mid, 0.2, 100, 1, 8, freqs_of_sigma(np.geomspace(0.5, 50.0, 64)))
    # borders and corners: a cell on the edge, then one whose profile is complete, in turns - the two share a workgroup
    ny, nx = zs.shape
    # (the corners, cells on the four edges, then cells 7 to 15 cells from the top and from the right: clipped, yet fitted)
    edge = np.concatenate([np.array([0, nx - 1, nx * (ny - 1), ny * nx - 1]), rng.integers(0, nx, 2),
                           rng.integers(0, ny, 2) * nx, rng.integers(0, ny, 2) * nx + nx - 1, (ny - 1) * nx + rng.integers(0, nx, 2),
                           rng.integers(7, 16, 4) * nx + rng.integers(0, nx, 4),
                           rng.integers(0, ny, 4) * nx + nx - 1 - rng.integers(7, 16, 4)])
    inner = rng.integers(30, 66, 19) * nx + rng.integers(30, 98, 19)
    mixed = np.empty(39, dtype=np.int64)
    mixed[0::2], mixed[1::2] = edge, inner
    add(NAMES[7], zs, 1.0, mixed, rng.uniform(-np.pi, np.pi, 39), 20, 2, 3, freqs_of_sigma(np.geomspace(0.5, 10.0, 12)), ms=6)
    # NaN cells: scattered holes under 30 cells of any orientation, then three cells at orientation 0 and swath 0 in rows of
    # their own - a hole at the centre point (j = -1 and 0 go), one at j = 1 and 2, where a shifted centre sits, and one
    # over the whole positive side (status 1)
    zn = zs.copy()
    zn[rng.random(zn.shape) < 0.004] = np.nan
    zn[8:14, :] = zs[8:14, :]
    zn[10, 60] = np.nan
    zn[12, 62] = np.nan
    zn[8, 61:] = np.nan
    holes = np.array([10 * nx + 60, 12 * nx + 60, 8 * nx + 60])
    add(NAMES[8], zn, 1.0, np.concatenate([rng.integers(20, 76, 30) * nx + rng.integers(20, 108, 30), holes]),
        np.concatenate([rng.uniform(-np.pi / 2, np.pi / 2, 30), np.zeros(3)]), 20, 0, 3,
        freqs_of_sigma(np.geomspace(0.5, 10.0, 12)), ms=6)
    add(NAMES[9], zs, 1.0, np.repeat(on[:5], 3)[::-1], 0.2, 30, 2, 4, freqs_of_sigma(np.geomspace(0.5, 15.0, 12)), delta=0.0)
    add(NAMES[10], zs, 1.0, on[:1], 0.2, 30, 2, 4, freqs_of_sigma(np.geomspace(0.5, 15.0, 12)))
    add(NAMES[11], zs, 1.0, on[:0], 0.2, 30, 2, 4, freqs_of_sigma(np.geomspace(0.5, 15.0, 12)))
    # no live pair: the narrowest trough the call takes, pi f de = 6, is one entry of 1, two of 2e-16 and, four points out,
    # 1e-250.  A hole over j = -4..3 leaves a column whose See underflows: the one frequency is dead and the row is 1 | 32
    zd = zs.copy()
    zd[40, 57:64] = np.nan
    add(NAMES[12], zd, 1.0, np.array([40 * nx + 60, 44 * nx + 60, 48 * nx + 61]), 0.0, 20, 0, 0, [6.0 / np.pi])
    _CASES = cases
    return cases
