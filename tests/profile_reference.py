"""numpy restatement of sc_fit_profiles (docs/profiles.md, include/scarplet_hip.h): the sampling formula written out,
``np.linalg.lstsq`` in float64 on the three columns, scipy's ``erf`` - and a second restatement of the fit alone in
``np.longdouble`` (Gram-Schmidt), the reference-side noise floor the GPU tolerances stand on."""
import numpy as np
from scipy.special import erf

ROW_FLOATS = ("kt", "kt_lo", "kt_hi", "a", "b", "c0", "sse", "rmse")


def sample_profile(z, r, c, sa, ca, h, w):
    """p_j (NaN where no sample of the point is valid) for j = -h..h at cell (r, c): the definition, to the letter."""
    ny, nx = z.shape
    j = np.arange(-h, h + 1, dtype=np.float64)
    acc = np.zeros(2 * h + 1)
    cnt = np.zeros(2 * h + 1, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for kk in range(-w, w + 1):                                    # ascending k: the order of the mean's sum
            k = np.float64(kk)
            rr = r + (k * ca - j * sa)
            cc = c + (j * ca + k * sa)
            inside = (rr >= 0) & (rr <= ny - 1) & (cc >= 0) & (cc <= nx - 1)
            rs, cs = np.where(inside, rr, 0.0), np.where(inside, cc, 0.0)
            r0 = np.minimum(np.floor(rs), ny - 2).astype(np.int64)
            c0 = np.minimum(np.floor(cs), nx - 2).astype(np.int64)
            fr, fc = rs - r0, cs - c0
            v = (z[r0, c0] * (1 - fc) + z[r0, c0 + 1] * fc) * (1 - fr) + (z[r0 + 1, c0] * (1 - fc) + z[r0 + 1, c0 + 1] * fc) * fr
            ok = inside & np.isfinite(v)
            acc = acc + np.where(ok, v, 0.0)
            cnt += ok
        return np.where(cnt > 0, acc / np.maximum(cnt, 1), np.nan)


def design(s, kt):
    return np.stack([np.ones_like(s), s, erf(s / (2 * np.sqrt(kt)))], axis=1)


def fit_age(s, p, kt):
    """((c0, b, a), sse, condition number of the column-scaled design matrix) of one age, float64 lstsq."""
    X = design(s, kt)
    coef = np.linalg.lstsq(X, p, rcond=None)[0]
    res = p - (coef[0] + coef[1] * s + coef[2] * X[:, 2])
    return coef, float(np.sum(res * res)), float(np.linalg.cond(X / np.linalg.norm(X, axis=0)))


def fit_age_longdouble(s, p, kt):
    """The same fit by Gram-Schmidt in np.longdouble (the erf column itself is scipy's float64)."""
    L = np.longdouble
    e = erf(s / (2 * np.sqrt(kt))).astype(L)
    s, p = s.astype(L), p.astype(L)
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


def choose(sse, n, delta):
    """(kt_index, lo_index, hi_index, status) from one cell's sse curve."""
    A = len(sse)
    best = int(np.argmin(sse))
    thr = sse[best] * (1.0 + delta / (n - 3))
    lo = hi = best
    while lo > 0 and sse[lo - 1] <= thr:
        lo -= 1
    while hi < A - 1 and sse[hi + 1] <= thr:
        hi += 1
    return best, lo, hi, (2 if lo == 0 else 0) + (4 if hi == A - 1 else 0)


def fit_cell(z, de, cell, sa, ca, h, w, ages, delta=1.0, min_samples=4, fit=fit_age):
    """One cell's row as a dict, plus 'curve' (sse per age), 'cond' (largest condition number) and 'ptp' (the
    profile's peak-to-peak range)."""
    ny, nx = z.shape
    r, c = divmod(int(cell), nx)
    p = sample_profile(z, float(r), float(c), sa, ca, h, w)
    j = np.arange(-h, h + 1)
    ok = ~np.isnan(p)
    n = int(ok.sum())
    row = {"cell": int(cell), "n": n, "kt_index": -1, "lo_index": -1, "hi_index": -1, "status": 1,
           "curve": np.full(len(ages), np.nan), "cond": 0.0, "ptp": np.nan}
    for f in ROW_FLOATS:
        row[f] = np.nan
    if int((ok & (j < 0)).sum()) < min_samples or int((ok & (j > 0)).sum()) < min_samples:
        return row
    s = (j.astype(np.float64) * de)[ok]
    pv = p[ok]
    fits = [fit(s, pv, kt) for kt in ages]
    sse = np.array([float(f[1]) for f in fits])
    best, lo, hi, status = choose(sse, n, delta)
    c0, b, a = (float(v) for v in fits[best][0])
    row.update(kt_index=best, lo_index=lo, hi_index=hi, status=status, kt=float(ages[best]), kt_lo=float(ages[lo]),
               kt_hi=float(ages[hi]), a=a, b=b, c0=c0, sse=sse[best], rmse=float(np.sqrt(sse[best] / (n - 3))),
               curve=sse, ptp=float(pv.max() - pv.min()))
    if fit is fit_age:
        row["cond"] = max(f[2] for f in fits)
    return row


def fit_profiles(z, de, cells, angle, h, w, ages, delta=1.0, min_samples=4, fit=fit_age):
    """Rows (a list of dicts) for ``cells`` with one orientation each; z float64, h and w in cells."""
    z = np.asarray(z, dtype=np.float64)
    ages = np.asarray(ages, dtype=np.float64)
    angle = np.broadcast_to(np.asarray(angle, dtype=np.float64), (len(cells),))
    sa, ca = np.sin(angle), np.cos(angle)
    return [fit_cell(z, de, cells[k], sa[k], ca[k], h, w, ages, delta, min_samples, fit) for k in range(len(cells))]


# ---- comparing a set of rows with the restatement -------------------------------------------------------------------
RTOL = 1e-9          # sse relative; c0, b h de, a relative to the profile's peak-to-peak range (see test_gpu_profiles)
COND_MAX = 1e3       # a condition on the inputs: the column-scaled design matrix of every compared fit
TIE_SHARE = 0.01     # cells whose index was decided inside RTOL, per case


def fit_cell_all(z, de, cell, sa, ca, h, w, ages, delta, min_samples):
    """fit_cell plus 'coefs' (A x 3: c0, b, a of every age) - what a row with another index is compared against."""
    row = fit_cell(z, de, cell, sa, ca, h, w, ages, delta, min_samples)
    if row["status"] != 1:
        ny, nx = z.shape
        r, c = divmod(int(cell), nx)
        p = sample_profile(z, float(r), float(c), sa, ca, h, w)
        ok = ~np.isnan(p)
        s = (np.arange(-h, h + 1).astype(np.float64) * de)[ok]
        row["coefs"] = np.array([fit_age(s, p[ok], kt)[0] for kt in ages])
    return row


def compare_rows(ref, got, h, de, delta):
    """``got`` (dicts with the row's fields and optionally 'curve') against ``ref`` (fit_cell_all rows).  Asserts what
    is exact or within RTOL; returns the figures: cells, fitted, ties (cells whose kt / lo / hi index differs and was
    decided within RTOL), the largest relative sse difference, the largest coefficient difference over the range,
    the largest condition number."""
    out = {"cells": len(ref), "fitted": 0, "ties": 0, "sse": 0.0, "coef": 0.0, "cond": 0.0}
    for r, g in zip(ref, got):
        assert int(g["n"]) == r["n"], (r["cell"], g["n"], r["n"])
        assert (int(g["status"]) & 1) == (r["status"] & 1), (r["cell"], g["status"], r["status"])
        if r["status"] == 1:
            assert int(g["kt_index"]) == -1 and all(np.isnan(g[f]) for f in ROW_FLOATS), r["cell"]
            continue
        out["fitted"] += 1
        assert r["cond"] <= COND_MAX, ("the inputs leave the tolerance's ground", r["cell"], r["cond"])
        out["cond"] = max(out["cond"], r["cond"])
        curve, n = r["curve"], r["n"]
        gi, glo, ghi = int(g["kt_index"]), int(g["lo_index"]), int(g["hi_index"])
        tie = False
        if gi != r["kt_index"]:
            assert abs(curve[gi] - r["sse"]) <= RTOL * r["sse"], (r["cell"], gi, r["kt_index"], curve[gi], r["sse"])
            tie = True
        thr = curve[gi] * (1.0 + delta / (n - 3))
        # a walk that parted: the index one side took and the other refused
        for gv, rv, i in ((glo, r["lo_index"], max(glo, r["lo_index"]) - 1), (ghi, r["hi_index"], min(ghi, r["hi_index"]) + 1)):
            if gv != rv:
                assert abs(curve[i] - thr) <= RTOL * thr, (r["cell"], gv, rv, curve[i], thr)
                tie = True
        if tie:
            out["ties"] += 1
        else:
            assert int(g["status"]) == r["status"], (r["cell"], g["status"], r["status"])
        ds = abs(float(g["sse"]) - curve[gi]) / curve[gi]
        c0, b, a = r["coefs"][gi]
        dc = max(abs(float(g["c0"]) - c0), abs(float(g["b"]) - b) * h * de, abs(float(g["a"]) - a)) / r["ptp"]
        if "curve" in g and g["curve"] is not None:
            ds = max(ds, float(np.max(np.abs(np.asarray(g["curve"], dtype=np.float64) - curve) / curve)))
        assert ds <= RTOL, (r["cell"], "sse", ds)
        assert dc <= RTOL, (r["cell"], "coefficients", dc)
        out["sse"], out["coef"] = max(out["sse"], ds), max(out["coef"], dc)
    assert out["ties"] <= TIE_SHARE * max(1, out["cells"]), out
    return out


# ---- the inputs of tests/test_gpu_profiles.py (and of the noise-floor test on the CPU) -------------------------------
def synthetic_z(n, **kw):
    from scarplet_amd import synthetic
    return np.asarray(synthetic.synthetic_scarp(n, **kw)._griddata, dtype=np.float64)


def scarp_cells(n, k, rng, spread=0.0, theta=0.2):
    """k cells on (within ``spread`` cells of) the scarp line of synthetic_scarp(n)."""
    x = np.linspace(-n / 2, n / 2, num=n)
    rows = rng.integers(n // 4, 3 * n // 4, k)
    # the line: -x cos(theta) + y sin(theta) = 0
    xc = x[rows] * np.tan(theta) + spread * rng.standard_normal(k)
    cols = np.clip(np.rint((xc + n / 2) * (n - 1) / n), 0, n - 1).astype(np.int64)
    return rows.astype(np.int64) * n + cols


def _golden_dem(name):
    import os
    f = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name))
    return f["z"].astype(np.float64), float(f["dx"])


def gpu_cases(big=True):
    """The cases as dicts: name, z, de, cells (int64), angle (one per cell), h, w (cells), ages, delta, min_samples,
    sample (indices of the cells compared with the restatement; None: all).  Seeded: the same on every box."""
    from scarplet_amd import _plan
    ages = _plan.age_grid()
    cases = []

    def add(name, z, de, cells, angle, h, w, kt=ages, delta=1.0, ms=4, sample=None):
        cells = np.ascontiguousarray(cells, dtype=np.int64)
        angle = np.ascontiguousarray(np.broadcast_to(np.asarray(angle, dtype=np.float64), cells.shape))
        cases.append(dict(name=name, z=z, de=float(de), cells=cells, angle=angle, h=h, w=w,
                          ages=np.asarray(kt, dtype=np.float64), delta=delta, min_samples=ms, sample=sample))

    rng = np.random.default_rng(20261016)
    z, de = _golden_dem("dem_carrizo.npz")
    cells = rng.integers(0, z.size, 300)
    ang = rng.uniform(-np.pi / 2, np.pi / 2, 300)
    add("carrizo h50 w2", z, de, cells, ang, 50, 2, ms=15)
    add("carrizo h50 w0", z, de, cells, ang, 50, 0, ms=15, delta=4.0)
    z, de = _golden_dem("dem_grandcanyon.npz")
    add("grandcanyon h100 w5", z, de, rng.integers(0, z.size, 300), rng.uniform(-np.pi, np.pi, 300), 100, 5, ms=20)
    z = synthetic_z(600)
    on = scarp_cells(600, 120, rng, spread=3.0)
    for h, w in ((100, 0), (100, 5), (30, 5), (15, 2)):
        add("synthetic h%d w%d" % (h, w), z, 1.0, on, 0.2 + 0.05 * rng.standard_normal(120), h, w, ms=min(h, 15))
    add("multiples of pi/4", z, 1.0, rng.integers(0, z.size, 180), np.tile(np.arange(-4, 5) * (np.pi / 4), 20), 30, 3, ms=20)
    add("repeated cells", z, 1.0, np.repeat(on[:7], 3)[::-1], 0.2, 100, 5, ms=15, delta=0.0)
    add("one age", z, 1.0, on[:60], 0.2, 100, 2, kt=[10.0], ms=15)
    add("64 ages", z, 1.0, on[:60], 0.2, 100, 2, kt=10 ** np.linspace(0, 3.4, 64), ms=15)
    # h = 2 with min_samples = 2 fits complete profiles only: five points, symmetric about j = 0, whose odd part
    # has two degrees of freedom - s and the erf of ANY age span it, so every age gives the same sse and the
    # choice among them is rounding.  One young age, then: n, sse and the coefficients are what can be compared.
    add("h2", z, 1.0, scarp_cells(600, 200, rng, spread=1.0), 0.2, 2, 1, kt=ages[:1], ms=2)
    add("one cell", z, 1.0, on[:1], 0.2, 100, 5, ms=15)
    add("no cell", z, 1.0, on[:0], 0.2, 100, 5, ms=15)
    # borders and corners: rows without a fit, and profiles with points missing
    n = 300
    zb = synthetic_z(n, seed=7)
    edge = np.concatenate([np.array([0, n - 1, n * (n - 1), n * n - 1]), rng.integers(0, n, 40),               # top row
                           rng.integers(0, n, 40) * n, rng.integers(0, n, 40) * n + n - 1,                     # sides
                           (n - 1) * n + rng.integers(0, n, 40),
                           rng.integers(0, 40, 60) * n + rng.integers(0, n, 60),                               # near the top
                           rng.integers(0, n, 60) * n + rng.integers(n - 40, n, 60)])                          # near the right
    add("borders and corners", zb, 1.0, edge, rng.uniform(-np.pi, np.pi, len(edge)), 100, 5, ms=20)
    # NaN cells: scattered, and a block
    zn = synthetic_z(400, seed=11).copy()
    zn[rng.random(zn.shape) < 0.004] = np.nan
    zn[180:200, 150:230] = np.nan
    add("NaN cells", zn, 1.0, rng.integers(0, zn.size, 250), rng.uniform(-np.pi / 2, np.pi / 2, 250), 40, 3, ms=20)
    if big:
        zz = synthetic_z(4096)
        mid = scarp_cells(4096, 48, rng, spread=20.0)
        add("h1024", zz, 1.0, mid, 0.2, 1024, 1, ms=100)
        cells = rng.integers(0, zz.size, 10 ** 6)
        add("a million cells", zz, 1.0, cells, 0.2 + 0.1 * rng.standard_normal(10 ** 6), 100, 5, ms=20,
            sample=np.sort(np.random.default_rng(5).choice(10 ** 6, 2000, replace=False)))
    return cases


def restate(case, fit=None):
    """The restatement's rows for the compared cells of a case (fit: None for fit_cell_all, else fit_cell with it)."""
    idx = np.arange(len(case["cells"])) if case["sample"] is None else case["sample"]
    sa, ca = np.sin(case["angle"]), np.cos(case["angle"])
    rows = []
    for k in idx:
        args = (case["z"], case["de"], case["cells"][k], sa[k], ca[k], case["h"], case["w"], case["ages"], case["delta"],
                case["min_samples"])
        rows.append(fit_cell_all(*args) if fit is None else fit_cell(*args, fit=fit))
    return idx, rows
