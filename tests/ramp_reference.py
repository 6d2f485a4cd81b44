"""numpy restatement of sc_fit_profiles_ramp (docs/profiles.md, "The initial slope"; include/scarplet_hip.h),
algebraically independent of the device's route: for EACH (cell, age, half-width) ``np.linalg.lstsq`` in float64 on the
three columns ``1, s, g`` handed to LAPACK equilibrated, the column ``g`` formed from the table of F as the definition
says - and a second restatement in ``np.longdouble`` (Gram-Schmidt; F, its erf and the column difference in longdouble
too), the reference-side noise floor the GPU tolerances stand on.  The profiles are
``profile_reference.sample_profile``'s, the walk of the interval ``profile_reference.choose``'s."""
import numpy as np
from scipy.special import erf

import profile_reference as pr

RTOL, COND_MAX, TIE_SHARE = pr.RTOL, pr.COND_MAX, pr.TIE_SHARE
FREE, SLOPE = 0, 1


# ---- the tables and the column ---------------------------------------------------------------------------------------
def ftab(h, M, de, ages):
    """F over x = -(h + M)..(h + M) and the ages, float64: (2 (h + M) + 1, A)."""
    X = (np.arange(-(h + M), h + M + 1).astype(np.float64) * de)[:, None]
    kt = np.asarray(ages, dtype=np.float64)[None, :]
    return X * erf(X / (2 * np.sqrt(kt))) + (2 * np.sqrt(kt / np.pi)) * np.exp(-(X * X) / (4 * kt))


# pi to the longdouble's last bit (np.pi is the float64)
_PI_L = np.longdouble(4) * np.arctan(np.longdouble(1))


def erf_longdouble(x):
    """erf in np.longdouble: 2 / sqrt(pi) exp(-x^2) sum_n 2^n x^(2n+1) / (1 3 5 ... (2n + 1)), a series of terms of one
    sign; beyond |x| = 7 the complement is below 1e-22 and the value is +-1."""
    L = np.longdouble
    x = np.asarray(x, dtype=L)
    ax = np.minimum(np.abs(x), L(7))
    term = ax.copy()
    total = ax.copy()
    for n in range(1, 400):
        term = term * (2 * ax * ax) / L(2 * n + 1)
        total = total + term
    val = (L(2) / np.sqrt(_PI_L)) * np.exp(-ax * ax) * total
    return np.sign(x) * np.where(np.abs(x) >= 7, L(1), val)


def ftab_longdouble(h, M, de, ages):
    L = np.longdouble
    X = (np.arange(-(h + M), h + M + 1).astype(L) * L(de))[:, None]
    kt = np.asarray(ages, dtype=np.float64).astype(L)[None, :]
    return X * erf_longdouble(X / (2 * np.sqrt(kt))) + (2 * np.sqrt(kt / _PI_L)) * np.exp(-(X * X) / (4 * kt))


_TABLES = {}


def _tables(h, M, de, ages, longdouble=False):
    """(the table of F, the erf table over j = -h..h) of a call, float64 or longdouble: built once per process."""
    ages = np.asarray(ages, dtype=np.float64)
    key = (h, M, float(de), ages.tobytes(), longdouble)
    if key not in _TABLES:
        L = np.longdouble if longdouble else np.float64
        arg = (np.arange(-h, h + 1).astype(L) * L(de))[:, None] / (2 * np.sqrt(ages.astype(L)))[None, :]
        _TABLES[key] = (ftab_longdouble(h, M, de, ages), erf_longdouble(arg)) if longdouble else (ftab(h, M, de, ages), erf(arg))
    return _TABLES[key]


def columns(j, h, M, de, ages, tab, etab):
    """e of every (age, half-width) at the valid points j: (A, M + 1, n).  m = 0 is the erf, m >= 1 the difference of the
    rows j + m and j - m of the table over 2 m de, formed in that order."""
    out = np.empty((tab.shape[1], M + 1, len(j)), dtype=tab.dtype)
    out[:, 0, :] = etab[j + h].T
    for m in range(1, M + 1):
        out[:, m, :] = ((tab[j + (h + M) + m] - tab[j + (h + M) - m]) / tab.dtype.type(2 * m * de)).T
    return out


def g_exact(s, kt, L):
    """g(s; kt, L) in float64 for any L >= 0 (the surface generator's)."""
    s = np.asarray(s, dtype=np.float64)
    if L == 0:
        return erf(s / (2 * np.sqrt(kt)))
    F = lambda x: x * erf(x / (2 * np.sqrt(kt))) + 2 * np.sqrt(kt / np.pi) * np.exp(-x * x / (4 * kt))
    return (F(s + L) - F(s - L)) / (2 * L)


# ---- the fit of one (age, half-width) --------------------------------------------------------------------------------
def fit_pair(s, p, e):
    """((c0, b, a), sse) of one column: float64 lstsq, handed to LAPACK equilibrated - p less its mean (the mean goes back
    into c0), every column at unit norm - which changes the solution in no way and keeps lstsq's own error at the size of
    the residuals, not of the elevations."""
    pm = p.sum() / len(p)
    X = np.stack([np.ones_like(s), s, e], axis=1)
    norm = np.linalg.norm(X, axis=0)
    coef = np.linalg.lstsq(X / norm, p - pm, rcond=None)[0] / norm
    coef[0] += pm
    res = p - (coef[0] + coef[1] * s + coef[2] * e)
    return coef, float(np.sum(res * res))


def fit_all_lstsq(s, p, E):
    """fit_pair over E (A, M + 1, n): coefs (A, M + 1, 3), sse (A, M + 1)."""
    A, M1, _ = E.shape
    coefs, grid = np.empty((A, M1, 3)), np.empty((A, M1))
    for i in range(A):
        for m in range(M1):
            coefs[i, m], grid[i, m] = fit_pair(s, p, E[i, m])
    return coefs, grid


def fit_all_longdouble(s, p, E):
    """The same fits by Gram-Schmidt in np.longdouble, every pair at once."""
    L = np.longdouble
    s, p, E = s.astype(L), p.astype(L), E.astype(L)
    n = L(len(s))
    sbar, pbar, ebar = s.sum() / n, p.sum() / n, E.sum(axis=-1, keepdims=True) / n
    sc = s - sbar
    sss = (sc * sc).sum()
    beta, gamma = (sc * (p - pbar)).sum() / sss, (sc * (E - ebar)).sum(axis=-1, keepdims=True) / sss
    e2, p2 = (E - ebar) - gamma * sc, (p - pbar) - beta * sc
    a = (e2 * p2).sum(axis=-1, keepdims=True) / (e2 * e2).sum(axis=-1, keepdims=True)
    b = beta - a * gamma
    c0 = pbar - a * ebar - b * sbar
    res = p - (c0 + b * s + a * E)
    return np.concatenate([c0, b, a], axis=-1), (res * res).sum(axis=-1)


def conds(s, E):
    """Condition numbers of the column-scaled design matrices of every pair: (A, M + 1)."""
    X = np.empty(E.shape + (3,))
    X[..., 0] = 1.0
    X[..., 1] = s
    X[..., 2] = E
    X = X / np.linalg.norm(X, axis=2, keepdims=True)
    sv = np.linalg.svd(X, compute_uv=False)
    return sv[..., 0] / sv[..., -1]


def profile_of(z, cell, sa, ca, h, w, min_samples):
    """(p, valid j, n, usable) of one cell."""
    r, c = divmod(int(cell), z.shape[1])
    p = pr.sample_profile(z, float(r), float(c), sa, ca, h, w)
    j = np.arange(-h, h + 1)
    ok = ~np.isnan(p)
    usable = int((ok & (j < 0)).sum()) >= min_samples and int((ok & (j > 0)).sum()) >= min_samples
    return p[ok], j[ok], int(ok.sum()), usable


def slopes_of(coefs, de):
    """The signed initial slope b + a / (m de) of every pair: (A, M + 1); copysign(inf, a) at m = 0."""
    M1 = coefs.shape[1]
    out = np.empty(coefs.shape[:2], dtype=coefs.dtype)
    out[:, 0] = np.copysign(np.inf, coefs[:, 0, 2].astype(np.float64))
    for m in range(1, M1):
        out[:, m] = coefs[:, m, 1] + coefs[:, m, 2] / coefs.dtype.type(m * de)
    return out


def pairs_of(z, de, cell, sa, ca, h, w, M, ages, min_samples=4, longdouble=False):
    """What does not depend on the mode: n, usable, and for a usable cell 'grid' (A x (M + 1): sse_im), 'coefs' (A x
    (M + 1) x 3: c0, b, a), 'slopes', 'cond' (the largest condition number; the float64 restatement alone) and 'ptp'."""
    p, j, n, usable = profile_of(z, cell, sa, ca, h, w, min_samples)
    out = {"cell": int(cell), "n": n, "usable": usable, "cond": 0.0, "ptp": np.nan}
    if not usable:
        return out
    s = j.astype(np.float64) * de
    E = columns(j, h, M, de, ages, *_tables(h, M, de, ages, longdouble))
    if longdouble:
        coefs, grid = fit_all_longdouble(s, p, E)
    else:
        coefs, grid = fit_all_lstsq(s, p, E)
        out["cond"] = float(conds(s, E).max())
    out.update(grid=grid, coefs=coefs, slopes=slopes_of(coefs, de), ptp=float(p.max() - p.min()))
    return out


def choose_cell(pairs, de, M, ages, mode=FREE, slope=None, delta=1.0):
    """One cell's row as a dict from pairs_of: the fields of sc_profile_ramp_fit, plus 'dof', 'keys' (A x (M + 1): what
    the choice per age compared, inf where a pair is no candidate), 'widths' (m_i), 'curve' (sse*)."""
    A = len(ages)
    n = pairs["n"]
    dof = n - 3 - (1 if mode == FREE and M > 0 else 0)
    row = dict(pairs, dof=dof, kt_index=-1, lo_index=-1, hi_index=-1, status=1, width_index=0, width=np.nan,
               initial_slope=np.nan, curve=np.full(A, np.nan), widths=np.zeros(A, dtype=np.int64))
    for f in pr.ROW_FLOATS:
        row[f] = np.nan
    if not pairs["usable"] or dof < 1:
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
    m = int(pick[best])
    c0, b, a = (float(v) for v in pairs["coefs"][best, m])
    sse = float(curve[best])
    row.update(keys=keys, widths=pick, curve=curve, kt_index=best, lo_index=lo, hi_index=hi,
               status=status + (8 if M > 0 and m == M else 0), width_index=m, width=m * de,
               initial_slope=float(pairs["slopes"][best, m]), kt=float(ages[best]), kt_lo=float(ages[lo]),
               kt_hi=float(ages[hi]), a=a, b=b, c0=c0, sse=sse, rmse=float(np.sqrt(sse / dof)))
    return row


def pairs_of_cells(z, de, cells, angle, h, w, M, ages, min_samples=4, longdouble=False):
    z = np.asarray(z, dtype=np.float64)
    ages = np.asarray(ages, dtype=np.float64)
    angle = np.broadcast_to(np.asarray(angle, dtype=np.float64), (len(cells),))
    sa, ca = np.sin(angle), np.cos(angle)
    return [pairs_of(z, de, cells[k], sa[k], ca[k], h, w, M, ages, min_samples, longdouble) for k in range(len(cells))]


def fit_profiles(z, de, cells, angle, h, w, M, ages, mode=FREE, slope=None, delta=1.0, min_samples=4, pairs=None):
    """Rows (a list of dicts) for ``cells`` with one orientation each; h, w and M in cells."""
    pairs = pairs_of_cells(z, de, cells, angle, h, w, M, ages, min_samples) if pairs is None else pairs
    return [choose_cell(q, de, M, np.asarray(ages, dtype=np.float64), mode, slope, delta) for q in pairs]


# ---- comparing the device's rows with the restatement ------------------------------------------------------------------
def compare_rows(ref, table, curve, widths, h, de, M, mode, slope, delta):
    """The device's table, (K, A) sse* curves and (K, A) half-widths against ``ref`` (choose_cell rows).  Asserts what is
    exact or within RTOL; returns the figures.  An m_i that differs from the restatement's must have been decided within
    RTOL by the restatement's own key - relative to the key with the width free (the key is an sse), to the given slope
    otherwise (the key is a distance between slopes of that size, and can itself be 0).  The curve and the indices are
    then judged at the device's m_i, on the restatement's sse.  A cell counts as a tie when an index or an m_i of it
    differs and was so decided."""
    out = {"cells": len(ref), "fitted": 0, "ties": 0, "sse": 0.0, "coef": 0.0, "cond": 0.0}
    for k, r in enumerate(ref):
        g = table[k]
        assert int(g["n"]) == r["n"], (r["cell"], g["n"], r["n"])
        assert (int(g["status"]) & 1) == (r["status"] & 1), (r["cell"], g["status"], r["status"])
        if r["status"] == 1:
            assert int(g["kt_index"]) == -1 and int(g["lo_index"]) == -1 and int(g["hi_index"]) == -1, r["cell"]
            assert all(np.isnan(g[f]) for f in pr.ROW_FLOATS) and np.isnan(g["height"]), r["cell"]
            assert int(g["width_index"]) == 0 and np.isnan(g["width"]) and np.isnan(g["initial_slope"]), r["cell"]
            assert np.isnan(curve[k]).all() and not widths[k].any()
            continue
        out["fitted"] += 1
        assert r["cond"] <= COND_MAX, ("the inputs leave the tolerance's ground", r["cell"], r["cond"])
        out["cond"] = max(out["cond"], r["cond"])
        A = len(r["curve"])
        mi = widths[k].astype(np.int64)
        assert mi.min() >= (1 if mode == SLOPE else 0) and mi.max() <= M, (r["cell"], mi)
        tie = False
        for i in np.flatnonzero(mi != r["widths"]):
            kd, kr = r["keys"][i, mi[i]], r["keys"][i, r["widths"][i]]
            assert abs(kd - kr) <= RTOL * (slope if mode == SLOPE else kr), (r["cell"], i, mi[i], r["widths"][i], kd, kr)
            tie = True
        cv, dof = r["grid"][np.arange(A), mi], r["dof"]
        ds = float(np.max(np.abs(curve[k] - cv) / cv))
        gi, glo, ghi = int(g["kt_index"]), int(g["lo_index"]), int(g["hi_index"])
        ri = int(np.argmin(cv))
        if gi != ri:
            assert abs(cv[gi] - cv[ri]) <= RTOL * cv[ri], (r["cell"], gi, ri, cv[gi], cv[ri])
            tie = True
        rb, rlo, rhi, _ = pr.choose(cv, dof + 3, delta)
        thr = cv[gi] * (1.0 + delta / dof)
        for gv, rv, i in ((glo, rlo, max(glo, rlo) - 1), (ghi, rhi, min(ghi, rhi) + 1)):
            if gv != rv:
                assert abs(cv[i] - thr) <= RTOL * thr, (r["cell"], gv, rv, cv[i], thr)
                tie = True
        m = int(g["width_index"])
        assert m == mi[gi] and float(g["width"]) == m * de, (r["cell"], m, mi[gi])
        assert int(g["status"]) == (2 if glo == 0 else 0) + (4 if ghi == A - 1 else 0) + (8 if M > 0 and m == M else 0)
        if tie:
            out["ties"] += 1
        else:
            assert int(g["status"]) == r["status"] and m == r["width_index"] and gi == r["kt_index"], (r["cell"], g["status"])
        ds = max(ds, abs(float(g["sse"]) - cv[gi]) / cv[gi])
        assert float(g["sse"]) == curve[k][gi]
        c0, b, a = r["coefs"][gi, m]
        dc = max(abs(float(g["c0"]) - c0), abs(float(g["b"]) - b) * h * de, abs(float(g["a"]) - a)) / r["ptp"]
        assert ds <= RTOL, (r["cell"], "sse", ds)
        assert dc <= RTOL, (r["cell"], "coefficients", dc)
        ga, gb = float(g["a"]), float(g["b"])
        want = np.copysign(np.inf, ga) if m == 0 else gb + ga / (m * de)
        assert float(g["initial_slope"]) == want, (r["cell"], g["initial_slope"], want)
        assert float(g["rmse"]) == float(np.sqrt(g["sse"] / dof)) and float(g["height"]) == 2.0 * ga
        out["sse"], out["coef"] = max(out["sse"], ds), max(out["coef"], dc)
    assert out["ties"] <= TIE_SHARE * max(1, out["cells"]), out
    return out


# ---- the surface ---------------------------------------------------------------------------------------------------------
def ramp_scarp(n, kt0, L, theta=0.2, noise=0.05, seed=20260101, b=0.01):
    """scarplet_amd.synthetic.synthetic_scarp with g(.; kt0, L) in place of the erf: n x n float64 that were float32, as
    a lidar GeoTIFF is.  Across the strike the profile is z = a g(s) + b s with a = 1, b = -0.01 (docs/profiles.md, "The
    sign of a")."""
    x = np.linspace(-n / 2, n / 2, num=n, dtype=np.float64)
    th = np.pi / 2 - theta
    yrot = -x[np.newaxis, :] * np.sin(th) + x[:, np.newaxis] * np.cos(th)
    z = -g_exact(yrot, kt0, L) + b * yrot
    z += noise * np.random.default_rng(seed).standard_normal((n, n))
    return z.astype(np.float32).astype(np.float64)


def line_cells(n=600, theta=0.2):
    """100 cells on the scarp's line of an n x n surface: rows n/4, n/4 + 3, ..., at the column where |yrot| is smallest
    (segment_reference.noisy_case's)."""
    x = np.linspace(-n / 2, n / 2, num=n)
    rows = np.arange(n // 4, 3 * n // 4, 3)
    yrot = -x[None, :] * np.cos(theta) + x[rows][:, None] * np.sin(theta)
    return rows.astype(np.int64) * n + np.argmin(np.abs(yrot), axis=1)


# ---- the recovery surface of docs/profiles.md ------------------------------------------------------------------------------
REC = dict(n=600, theta=0.2, L=6, index=10, noise=0.02, h=100, w=2, M=8, slope=abs(-0.01 + 1.0 / 6.0))


def recovery_case(noise=REC["noise"]):
    """(z, cells, theta, ages): a ramp of half-width 6 cells diffused for ages[10], 100 cells on its line."""
    from scarplet_amd import _plan
    ages = _plan.age_grid()
    z = ramp_scarp(REC["n"], float(ages[REC["index"]]), REC["L"], REC["theta"], noise)
    return z, line_cells(REC["n"], REC["theta"]), REC["theta"], ages


# ---- the inputs of tests/test_gpu_ramp.py (and of the restatements' agreement on the CPU) ------------------------------------
# how far each case's age grid goes (the number of default ages, or the exponent of the last of the 64): chosen on the CPU
# so that no compared (age, half-width) passes COND_MAX and - the narrower of the two here - the float64 restatement and its
# longdouble twin agree within RTOL / 100 in every sse and coefficient: the rounding of the table's difference is what the
# old ages of short profiles amplify (docs/profiles.md, "The initial slope"; tests/test_ramp_host.py)
NA = {"h100 w0 M8": 35, "h100 w5 M1": 35, "h30 w5 M4": 32, "64 ages M1": 3.4, "repeated cells": 35, "M = h - min_samples": 25,
      "de 2": 35, "borders and corners": 35, "NaN cells": 33}
NAMES = ["h100 w0 M8", "h100 w5 M1", "h30 w5 M4", "64 ages M1", "one age M8", "M = h - min_samples", "de 2", "repeated cells",
         "no cell", "borders and corners", "NaN cells", "dof < 1"]


def gpu_cases():
    """The cases as dicts: name, z, de, cells, angle, h, w, M, ages, delta, min_samples, slope (the given slope of the
    run in that mode; None: the case runs with the width free alone).  Seeded: the same on every box."""
    from scarplet_amd import _plan
    ages = _plan.age_grid()
    cases = []

    def add(name, z, de, cells, angle, h, w, M, kt, slope=0.3, delta=1.0, ms=4):
        cells = np.ascontiguousarray(cells, dtype=np.int64)
        angle = np.ascontiguousarray(np.broadcast_to(np.asarray(angle, dtype=np.float64), cells.shape))
        cases.append(dict(name=name, z=z, de=float(de), cells=cells, angle=angle, h=h, w=w, M=M,
                          ages=np.asarray(kt, dtype=np.float64), delta=delta, min_samples=ms, slope=slope))

    rng = np.random.default_rng(20261020)
    z = ramp_scarp(600, 10.0, 4.0)
    on = pr.scarp_cells(600, 32, rng, spread=3.0)
    ang = 0.2 + 0.05 * rng.standard_normal(32)
    # 315 pairs: 5 rounds, the last one partial, the table in LDS
    add("h100 w0 M8", z, 1.0, on, ang, 100, 0, 8, ages[:NA["h100 w0 M8"]], ms=15)
    add("h100 w5 M1", z, 1.0, on, ang, 100, 5, 1, ages[:NA["h100 w5 M1"]], slope=0.9, ms=15)
    add("h30 w5 M4", z, 1.0, on, ang, 30, 5, 4, ages[:NA["h30 w5 M4"]], ms=15)
    # 128 pairs, no two lanes of a round share an age; 203 rows of 64 ages are 104 KB: the table in global memory
    add("64 ages M1", z, 1.0, on[:12], 0.2, 100, 2, 1, 10 ** np.linspace(0, NA["64 ages M1"], 64), slope=0.9, ms=15)
    # nine pairs of one age: the argmin across six shuffle steps
    add("one age M8", z, 1.0, on[:30], 0.2, 100, 2, 8, [10.0], ms=15)
    # the whole range the call accepts
    add("M = h - min_samples", z, 1.0, on[:20], 0.2, 12, 1, 8, ages[:NA["M = h - min_samples"]], ms=4)
    z2 = ramp_scarp(300, 40.0, 8.0, seed=5)                                # in data units of a 2 m grid: L = 4 cells
    add("de 2", z2, 2.0, pr.scarp_cells(300, 20, rng, spread=2.0), 0.2 + 0.05 * rng.standard_normal(20), 50, 2, 6,
        ages[:NA["de 2"]], slope=0.15, ms=10)
    add("repeated cells", z, 1.0, np.repeat(on[:5], 3)[::-1], 0.2, 100, 5, 4, ages[:NA["repeated cells"]], ms=15, delta=0.0)
    add("no cell", z, 1.0, on[:0], 0.2, 100, 5, 8, ages, ms=15)
    n = 300
    zb = ramp_scarp(n, 10.0, 3.0, seed=7)
    edge = np.concatenate([np.array([0, n - 1, n * (n - 1), n * n - 1]), rng.integers(0, n, 8), rng.integers(0, n, 8) * n,
                           rng.integers(0, n, 8) * n + n - 1, (n - 1) * n + rng.integers(0, n, 8),
                           rng.integers(0, 40, 16) * n + rng.integers(0, n, 16),
                           rng.integers(0, n, 16) * n + rng.integers(n - 40, n, 16)])
    add("borders and corners", zb, 1.0, edge, rng.uniform(-np.pi, np.pi, len(edge)), 100, 5, 3, ages[:NA["borders and corners"]],
        ms=20)
    zn = ramp_scarp(400, 10.0, 3.0, seed=11)
    zn[rng.random(zn.shape) < 0.004] = np.nan
    zn[180:200, 150:230] = np.nan
    add("NaN cells", zn, 1.0, rng.integers(0, zn.size, 60), rng.uniform(-np.pi / 2, np.pi / 2, 60), 40, 3, 3,
        ages[:NA["NaN cells"]], ms=20)
    # A cell with dof < 1 where the width is free: h = 3 and min_samples = 2 leave M = 1; the cell two columns off the right
    # border, itself NaN, at orientation 0 keeps j = -3, -2, 1, 2 (a NaN takes the two samples that read it, j = 3 lies
    # outside): n = 4, two on either side, dof = 4 - 3 - 1.  Next to it cells with all seven points.  Two young ages, the
    # width free alone: with the slope given the cell has dof = 1, four points for three coefficients
    zd = ramp_scarp(64, 1.0, 1.0, theta=0.0, noise=0.01, seed=3)
    zd[20, 61] = np.nan
    add("dof < 1", zd, 1.0, np.array([20 * 64 + 61, 31 * 64 + 30, 32 * 64 + 31, 33 * 64 + 32]), 0.0, 3, 0, 1, [1.0, 1.5],
        slope=None, ms=2)
    assert [c["name"] for c in cases] == NAMES
    return cases


_PAIRS = {}


def case_pairs(case, longdouble=False):
    """pairs_of every cell of a case, computed once per process."""
    key = (case["name"], longdouble)
    if key not in _PAIRS:
        _PAIRS[key] = pairs_of_cells(case["z"], case["de"], case["cells"], case["angle"], case["h"], case["w"], case["M"],
                                     case["ages"], case["min_samples"], longdouble)
    return _PAIRS[key]


def restate(case, mode, longdouble=False):
    return [choose_cell(q, case["de"], case["M"], case["ages"], mode, case["slope"], case["delta"])
            for q in case_pairs(case, longdouble)]
