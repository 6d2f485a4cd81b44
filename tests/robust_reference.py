"""numpy restatement of sc_fit_profiles_robust (docs/profiles.md, "Weights and robust fits"): the weighted samples
written out, ``np.linalg.lstsq`` in float64 on the three weighted columns, the exact order statistic by ``np.sort`` -
and a second restatement of the weighted fit alone in ``np.longdouble`` (Gram-Schmidt), the reference-side noise floor
the GPU tolerance stands on.  The samples of a call without a weight plane and the case generators are those of
tests/profile_reference.py."""
import numpy as np
from scipy.special import erf

import profile_reference as pr
from profile_reference import RTOL, COND_MAX, TIE_SHARE, ROW_FLOATS, sample_profile      # noqa: F401

HUBER_K, TUKEY_K = 1.345, 4.685
MAD = 1.4826
FLOATS = ROW_FLOATS + ("loss", "scale")


# ---- samples ---------------------------------------------------------------------------------------------------------
def _bilinear(z, rr, cc, inside):
    ny, nx = z.shape
    rs, cs = np.where(inside, rr, 0.0), np.where(inside, cc, 0.0)
    r0 = np.minimum(np.floor(rs), ny - 2).astype(np.int64)
    c0 = np.minimum(np.floor(cs), nx - 2).astype(np.int64)
    fr, fc = rs - r0, cs - c0
    return (z[r0, c0] * (1 - fc) + z[r0, c0 + 1] * fc) * (1 - fr) + (z[r0 + 1, c0] * (1 - fc) + z[r0 + 1, c0 + 1] * fc) * fr


def sample_weighted(z, wt, r, c, sa, ca, h, w):
    """(p_j, u_j) for j = -h..h at cell (r, c).  Without a plane p is sample_profile's and u is 1.  With one, a sample is
    valid when the elevation sample is valid and the weight sample - the same formula at the same position - is finite
    and >= 0; p and u are the means over the same valid k in ascending k; a point whose u is not > 0 is missing (NaN)."""
    if wt is None:
        p = sample_profile(z, r, c, sa, ca, h, w)
        return p, np.where(np.isnan(p), np.nan, 1.0)
    ny, nx = z.shape
    j = np.arange(-h, h + 1, dtype=np.float64)
    accp, accu = np.zeros(2 * h + 1), np.zeros(2 * h + 1)
    cnt = np.zeros(2 * h + 1, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for kk in range(-w, w + 1):
            k = np.float64(kk)
            rr = r + (k * ca - j * sa)
            cc = c + (j * ca + k * sa)
            inside = (rr >= 0) & (rr <= ny - 1) & (cc >= 0) & (cc <= nx - 1)
            v, g = _bilinear(z, rr, cc, inside), _bilinear(wt, rr, cc, inside)
            ok = inside & np.isfinite(v) & np.isfinite(g) & (g >= 0)
            accp = accp + np.where(ok, v, 0.0)
            accu = accu + np.where(ok, g, 0.0)
            cnt += ok
        p = np.where(cnt > 0, accp / np.maximum(cnt, 1), np.nan)
        u = np.where(cnt > 0, accu / np.maximum(cnt, 1), np.nan)
        gone = ~(u > 0)
        return np.where(gone, np.nan, p), np.where(gone, np.nan, u)


# ---- the weighted fit of one age -------------------------------------------------------------------------------------
def wfit(s, p, e, q):
    """((c0, b, a), See of the weighted columns) of one age: float64 lstsq on the rows scaled by sqrt(q).  The problem is
    handed to LAPACK equilibrated - p less its weighted mean (the mean goes back into c0), every column at unit norm -
    which changes the solution in no way and keeps lstsq's own error at the size of the residuals, not of the elevations."""
    g = np.sqrt(q)
    W = q.sum()
    pm = (q * p).sum() / W
    X = np.stack([np.ones_like(s), s, e], axis=1) * g[:, None]
    norm = np.linalg.norm(X, axis=0)
    coef = np.linalg.lstsq(X / norm, (p - pm) * g, rcond=None)[0] / norm
    coef[0] += pm
    sc = s - (q * s).sum() / W
    ec = e - (q * e).sum() / W
    e2 = ec - ((q * sc * ec).sum() / (q * sc * sc).sum()) * sc
    return coef, float((q * e2 * e2).sum())


def wfit_longdouble(s, p, e, q):
    """The same fit by weighted Gram-Schmidt in np.longdouble (e itself is scipy's float64)."""
    L = np.longdouble
    s, p, e, q = s.astype(L), p.astype(L), e.astype(L), q.astype(L)
    W = q.sum()
    sbar, pbar, ebar = (q * s).sum() / W, (q * p).sum() / W, (q * e).sum() / W
    sc = s - sbar
    sss = (q * sc * sc).sum()
    beta, gamma = (q * sc * (p - pbar)).sum() / sss, (q * sc * (e - ebar)).sum() / sss
    e2, p2 = (e - ebar) - gamma * sc, (p - pbar) - beta * sc
    see = (q * e2 * e2).sum()
    a = (q * e2 * p2).sum() / see
    b = beta - a * gamma
    c0 = pbar - a * ebar - b * sbar
    return np.array([c0, b, a], dtype=L), see


def factor(loss, r, c):
    """f(|r|): the robust weight of a residual."""
    x = np.abs(r)
    with np.errstate(divide="ignore", invalid="ignore"):
        if loss == "huber":
            return np.where(x <= c, 1.0, c / x)
        return np.where(x < c, (1.0 - (x / c) ** 2) ** 2, 0.0)


def rho(loss, r, c):
    x = np.abs(r)
    if loss == "huber":
        return np.where(x <= c, r * r, 2.0 * c * x - c * c)
    return np.where(x < c, (c * c / 3.0) * (1.0 - (1.0 - (r / c) ** 2) ** 3), c * c / 3.0)


def choose(curve, n, delta):
    """(kt_index, lo_index, hi_index, status) from one cell's loss curve; a NaN never wins and ends a walk."""
    A = len(curve)
    best = int(np.argmin(np.where(np.isnan(curve), np.inf, curve)))
    thr = curve[best] * (1.0 + delta / (n - 3))
    lo = hi = best
    while lo > 0 and curve[lo - 1] <= thr:
        lo -= 1
    while hi < A - 1 and curve[hi + 1] <= thr:
        hi += 1
    return best, lo, hi, (2 if lo == 0 else 0) + (4 if hi == A - 1 else 0)


def _cond(s, e, q):
    X = np.stack([np.ones_like(s), s, e], axis=1) * np.sqrt(q)[:, None]
    X = X[q > 0]
    return float(np.linalg.cond(X / np.linalg.norm(X, axis=0)))


def fit_cell(z, wt, de, cell, sa, ca, h, w, ages, delta=1.0, min_samples=4, robust=None, tuning=None, iterations=8,
             robust_scale=None, fit=wfit, force_ls=None, cond=True):
    """One cell's row as a dict: the fields of sc_profile_robust_fit, plus 'curve' (the loss per age), 'coefs' (A x 3: c0,
    b, a of every age's final fit), 'sse0' (the curve of iterate 0), 'cond' (the largest condition number of the weighted,
    column-scaled design matrices of iterate 0 and of the final iterate) and 'ptp' (the profile's range).  ``force_ls``
    takes ls_index as given: what a row whose ls_index was a tie is compared against."""
    ny, nx = z.shape
    A = len(ages)
    r_, c_ = divmod(int(cell), nx)
    p, u = sample_weighted(z, wt, float(r_), float(c_), sa, ca, h, w)
    j = np.arange(-h, h + 1)
    ok = ~np.isnan(p)
    n = int(ok.sum())
    row = {"cell": int(cell), "n": n, "kt_index": -1, "lo_index": -1, "hi_index": -1, "status": 1, "n_down": 0,
           "ls_index": -1, "curve": np.full(A, np.nan), "sse0": np.full(A, np.nan), "cond": 0.0, "ptp": np.nan,
           "coefs": np.full((A, 3), np.nan)}
    for f in FLOATS:
        row[f] = np.nan
    if int((ok & (j < 0)).sum()) < min_samples or int((ok & (j > 0)).sum()) < min_samples:
        return row
    jv = j[ok]
    s, pv, uv = jv.astype(np.float64) * de, p[ok], u[ok]
    E = [erf(s / (2 * np.sqrt(kt))) for kt in ages]
    F = np.float64 if fit is wfit else np.longdouble
    resid = lambda co, e: pv.astype(F) - ((co[0] + co[1] * s.astype(F)) + co[2] * e.astype(F))
    # iterate 0: the weighted least squares fit of every age
    coefs = [fit(s, pv, e, uv)[0] for e in E]
    res = [resid(co, e) for co, e in zip(coefs, E)]
    sse0 = np.array([float((uv * r * r).sum()) for r in res])
    row["sse0"] = sse0
    conds = [_cond(s, e, uv) for e in E] if cond and fit is wfit else [0.0]
    if np.isnan(sse0).all():
        row["status"] = 1 | 32
        return row
    ls = int(np.argmin(np.where(np.isnan(sse0), np.inf, sse0))) if force_ls is None else int(force_ls)
    curve, sigma, flag = sse0, np.nan, 0
    if robust is not None:
        k = float(tuning) if tuning is not None else (HUBER_K if robust == "huber" else TUKEY_K)
        sigma = float(robust_scale) if robust_scale is not None else float(MAD * np.sort(np.abs(res[ls]).astype(np.float64))[(n - 1) // 2])
        if not sigma > 0:
            flag = 16
        else:
            c = k * sigma
            curve = np.full(A, np.nan)
            for i, e in enumerate(E):
                co, r, dead = coefs[i], res[i], False
                for _ in range(iterations):
                    q = uv * factor(robust, r.astype(np.float64), c)
                    if int(((q > 0) & (jv < 0)).sum()) < min_samples or int(((q > 0) & (jv > 0)).sum()) < min_samples:
                        dead = True
                        break
                    co, see = fit(s, pv, e, q)
                    if not see > 0:
                        dead = True
                        break
                    r = resid(co, e)
                if dead:
                    coefs[i], res[i] = np.full(3, np.nan), np.full(len(s), np.nan)
                    continue
                coefs[i], res[i] = co, r
                curve[i] = float((uv * rho(robust, r, F(c))).sum())
                if cond and fit is wfit:
                    conds.append(_cond(s, e, q))
            if np.isnan(curve).all():
                row["status"] = 1 | 32
                row["scale"] = sigma
                return row
    best, lo, hi, status = choose(curve, n, delta)
    c0, b, a = (float(v) for v in coefs[best])
    sse = float((uv * res[best] * res[best]).sum())
    down = 0
    if robust is not None and not flag:
        down = int((factor(robust, res[best].astype(np.float64), k * sigma) < 1).sum())
    row.update(kt_index=best, lo_index=lo, hi_index=hi, status=status | flag, kt=float(ages[best]), kt_lo=float(ages[lo]),
               kt_hi=float(ages[hi]), a=a, b=b, c0=c0, sse=sse, loss=float(curve[best]),
               rmse=float(np.sqrt(curve[best] / (n - 3))), scale=sigma, n_down=down, ls_index=ls, curve=curve,
               coefs=np.array([[float(v) for v in co] for co in coefs]), cond=max(conds), ptp=float(pv.max() - pv.min()))
    return row


def fit_profiles(z, wt, de, cells, angle, h, w, ages, **kw):
    """Rows (a list of dicts) for ``cells`` with one orientation each; z (and wt) float64, h and w in cells."""
    z = np.asarray(z, dtype=np.float64)
    wt = None if wt is None else np.asarray(wt, dtype=np.float64)
    ages = np.asarray(ages, dtype=np.float64)
    angle = np.broadcast_to(np.asarray(angle, dtype=np.float64), (len(cells),))
    sa, ca = np.sin(angle), np.cos(angle)
    return [fit_cell(z, wt, de, cells[k], sa[k], ca[k], h, w, ages, **kw) for k in range(len(cells))]


# ---- comparing a set of rows with the restatement -----------------------------------------------------------------------
def compare_rows(case, ref, got):
    """``got`` (dicts with the row's fields and 'curve') against ``ref`` (fit_cell rows of ``case``), scaled as
    profile_reference.compare_rows scales: the loss, the sse, the curve and the scale relative, the coefficients over the
    profile's range, n, n_down and the status exact, the indices equal except for ties decided inside RTOL (a row whose
    ls_index was such a tie is compared with the restatement at the device's ls_index).  Returns the figures."""
    h, de, delta = case["h"], case["de"], case["delta"]
    out = {"cells": len(ref), "fitted": 0, "ties": 0, "loss": 0.0, "coef": 0.0, "scale": 0.0, "cond": 0.0}
    sa, ca = np.sin(case["angle"]), np.cos(case["angle"])
    for r, g in zip(ref, got):
        cell = r["cell"]
        assert int(g["n"]) == r["n"], (cell, g["n"], r["n"])
        assert (int(g["status"]) & 33) == (r["status"] & 33), (cell, g["status"], r["status"])
        if r["status"] & 1:
            assert int(g["kt_index"]) == -1 and int(g["ls_index"]) == -1 and int(g["n_down"]) == 0, cell
            assert all(np.isnan(g[f]) for f in FLOATS if f != "scale"), cell
            continue
        out["fitted"] += 1
        tie = False
        if int(g["ls_index"]) != r["ls_index"]:
            m = r["sse0"][r["ls_index"]]
            assert abs(r["sse0"][int(g["ls_index"])] - m) <= RTOL * m, (cell, "ls_index", g["ls_index"], r["ls_index"])
            tie = True
            r = fit_cell(case["z"], case.get("weights"), de, cell, sa[r["k"]], ca[r["k"]], h, case["w"], case["ages"], delta,
                         case["min_samples"], force_ls=int(g["ls_index"]), **case["robust"])
        assert r["cond"] <= COND_MAX, ("the inputs leave the tolerance's ground", cell, r["cond"])
        out["cond"] = max(out["cond"], r["cond"])
        assert (int(g["status"]) & 16) == (r["status"] & 16), (cell, g["status"], r["status"])
        curve, n = r["curve"], r["n"]
        gi, glo, ghi = int(g["kt_index"]), int(g["lo_index"]), int(g["hi_index"])
        if gi != r["kt_index"]:
            assert abs(curve[gi] - r["loss"]) <= RTOL * r["loss"], (cell, gi, r["kt_index"], curve[gi], r["loss"])
            tie = True
        thr = curve[gi] * (1.0 + delta / (n - 3))
        for gv, rv, i in ((glo, r["lo_index"], max(glo, r["lo_index"]) - 1), (ghi, r["hi_index"], min(ghi, r["hi_index"]) + 1)):
            if gv != rv:
                assert abs(curve[i] - thr) <= RTOL * thr, (cell, gv, rv, curve[i], thr)
                tie = True
        if tie:
            out["ties"] += 1
        else:
            assert int(g["status"]) == r["status"], (cell, g["status"], r["status"])
            assert int(g["n_down"]) == r["n_down"], (cell, g["n_down"], r["n_down"])
        gc = np.asarray(g["curve"], dtype=np.float64)
        assert np.array_equal(np.isnan(gc), np.isnan(curve)), (cell, "NaN ages")
        live = ~np.isnan(curve)
        dl = float(np.max(np.abs(gc[live] - curve[live]) / curve[live]))
        dl = max(dl, abs(float(g["loss"]) - curve[gi]) / curve[gi])
        if gi == r["kt_index"]:
            dl = max(dl, abs(float(g["sse"]) - r["sse"]) / r["sse"])
        c0, b, a = r["coefs"][gi]
        dc = max(abs(float(g["c0"]) - c0), abs(float(g["b"]) - b) * h * de, abs(float(g["a"]) - a)) / r["ptp"]
        dsig = 0.0
        if not np.isnan(r["scale"]):
            dsig = abs(float(g["scale"]) - r["scale"]) / r["scale"] if r["scale"] > 0 else abs(float(g["scale"]))
        else:
            assert np.isnan(g["scale"]), cell
        assert dl <= RTOL, (cell, "loss", dl)
        assert dc <= RTOL, (cell, "coefficients", dc)
        assert dsig <= RTOL, (cell, "scale", dsig)
        out["loss"], out["coef"], out["scale"] = max(out["loss"], dl), max(out["coef"], dc), max(out["scale"], dsig)
    assert out["ties"] <= TIE_SHARE * max(1, out["cells"]), out
    return out


# ---- the pit surface: what the robust fit is for ---------------------------------------------------------------------
# synthetic_scarp(600) (kt0 = 10: index 10 of the default age grid) with PIT_COUNT Gaussian pits dug into it -
# z -= depth exp(-((r - r0)^2 + (c - c0)^2) / (2 width^2)) within 6 widths of the centre, depth uniform in 0.3..0.8, width uniform in 2..4 cells, the
# centres uniform over the grid, all from default_rng(PIT_SEED) in the order centres' rows, centres' columns, depths,
# widths - and PIT_CELLS cells on the scarp line from the same generator, cut at the scarp's own strike.
PIT_SEED, PIT_COUNT, PIT_CELLS, PIT_TRUE_INDEX = 20261019, 400, 100, 10


def pit_surface(n=600, seed=PIT_SEED, count=PIT_COUNT):
    z = pr.synthetic_z(n).copy()
    rng = np.random.default_rng(seed)
    r0, c0 = rng.uniform(0, n, count), rng.uniform(0, n, count)
    depth, width = rng.uniform(0.3, 0.8, count), rng.uniform(2.0, 4.0, count)
    rr, cc = np.arange(n, dtype=np.float64)[:, None], np.arange(n, dtype=np.float64)[None, :]
    for k in range(count):
        lo_r, hi_r = max(0, int(r0[k] - 6 * width[k])), min(n, int(r0[k] + 6 * width[k]) + 2)
        lo_c, hi_c = max(0, int(c0[k] - 6 * width[k])), min(n, int(c0[k] + 6 * width[k]) + 2)
        d2 = (rr[lo_r:hi_r] - r0[k]) ** 2 + (cc[:, lo_c:hi_c] - c0[k]) ** 2
        z[lo_r:hi_r, lo_c:hi_c] -= depth[k] * np.exp(-d2 / (2.0 * width[k] ** 2))
    cells = pr.scarp_cells(n, PIT_CELLS, rng)
    return z, cells


def case(name, z, de, cells, angle, h, w, ages=None, delta=1.0, ms=4, weights=None, **robust):
    from scarplet_amd import _plan
    cells = np.ascontiguousarray(cells, dtype=np.int64)
    angle = np.ascontiguousarray(np.broadcast_to(np.asarray(angle, dtype=np.float64), cells.shape))
    return dict(name=name, z=z, de=float(de), cells=cells, angle=angle, h=h, w=w,
                ages=np.asarray(_plan.age_grid() if ages is None else ages, dtype=np.float64), delta=delta, min_samples=ms,
                weights=weights, robust=robust)


def pit_case(**robust):
    z, cells = pit_surface()
    return case("pit surface", z, 1.0, cells, 0.2, 100, 2, ms=15, **robust)


def restate(c, fit=wfit, cond=True):
    """The restatement's rows for a case (each with 'k', its position in the case)."""
    sa, ca = np.sin(c["angle"]), np.cos(c["angle"])
    rows = []
    for k in range(len(c["cells"])):
        row = fit_cell(c["z"], c["weights"], c["de"], c["cells"][k], sa[k], ca[k], c["h"], c["w"], c["ages"], c["delta"],
                       c["min_samples"], fit=fit, cond=cond, **c["robust"])
        row["k"] = k
        rows.append(row)
    return rows


def share_on(rows, index=PIT_TRUE_INDEX):
    return int(sum(1 for r in rows if int(r["kt_index"]) == index))


# ---- the inputs of tests/test_gpu_robust.py (and of the noise-floor test on the CPU) ---------------------------------------
def gpu_cases(loss):
    """The cases of one loss ("huber" or "tukey") as case() makes them, by name.  Seeded: the same on every box."""
    rng = np.random.default_rng(20261019)
    out = {}

    def add(name, *a, **kw):
        kw.setdefault("robust", loss)
        out[name] = case(name, *a, **kw)

    c = pit_case(robust=loss)
    out[c["name"]] = c
    z, de = pr._golden_dem("dem_carrizo.npz")
    add("carrizo h50 w2", z, de, rng.integers(0, z.size, 150), rng.uniform(-np.pi / 2, np.pi / 2, 150), 50, 2, ms=15)
    z = pr.synthetic_z(600)
    on = pr.scarp_cells(600, 40, rng, spread=3.0)
    ang = 0.2 + 0.05 * rng.standard_normal(40)
    add("one age", z, 1.0, on, ang, 100, 2, ages=[10.0], ms=15, iterations=5)
    add("64 ages", z, 1.0, on, ang, 100, 2, ages=10 ** np.linspace(0, 3.4, 64), ms=15, iterations=3)   # the table in global memory
    for h in (31, 32, 15):                                                 # 63, 65 and 31 points: a lane round and its edges
        # (at h = 15 the oldest ages are all but a line over the profile: the grid ends where COND_MAX would)
        add("h%d" % h, z, 1.0, on, ang, h, 2, ages=None if h > 15 else 10 ** np.linspace(0, 2.7, 28), ms=min(h, 15) - 3, iterations=4)
    parent = {c["name"]: c for c in pr.gpu_cases(big=False)}
    for name in ("borders and corners", "NaN cells"):
        p = parent[name]
        add(name, p["z"], p["de"], p["cells"], p["angle"], p["h"], p["w"], ages=p["ages"], delta=p["delta"], ms=p["min_samples"],
            iterations=3)
    for k in (0, 1, 5):
        add("K = %d" % k, z, 1.0, on[:k], ang[:k], 100, 5, ms=15, iterations=2)
    add("robust_scale given", z, 1.0, on, ang, 100, 2, ms=15, robust_scale=0.08, tuning=2.0, iterations=6)
    if loss == "tukey":                                                    # every point beyond c at once: status 1 | 32
        add("no age survives", z, 1.0, on[:8], ang[:8], 100, 2, ms=15, robust_scale=1e-9, iterations=2)
    # weight planes: a 0 / 1 plane that masks a strip beside the scarp line (a road), a random positive plane, and one with
    # NaN cells scattered and in a block
    cc = np.arange(600)[None, :] - (300 + (np.arange(600)[:, None] - 300) * np.tan(0.2))
    strip = np.where((cc > 20) & (cc < 32), 0.0, 1.0) * np.ones((600, 600))
    add("weights: a strip of zeros", z, 1.0, on, ang, 100, 2, ms=15, weights=strip, iterations=4)
    add("weights: random positive", z, 1.0, on, ang, 60, 3, ms=15, weights=rng.uniform(0.2, 3.0, z.shape), iterations=4)
    holes = rng.uniform(0.5, 1.5, z.shape)
    holes[rng.random(z.shape) < 0.004] = np.nan
    holes[280:300, 250:330] = np.nan
    add("weights: NaN cells", z, 1.0, on, ang, 60, 3, ms=15, weights=holes, iterations=4)
    add("weights alone", z, 1.0, on, ang, 60, 3, ms=15, weights=rng.uniform(0.2, 3.0, z.shape), robust=None)
    return out
