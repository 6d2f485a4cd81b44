"""numpy restatement of sc_fit_profiles_refine (docs/profiles.md, "Continuous ages"; include/scarplet_hip.h): the plain
restatement of tests/profile_reference.py, then the brackets, the candidates and the picks of the definition written out -
``profile_reference.fit_age`` (float64 ``lstsq``) per candidate, or ``fit_age_longdouble`` for the second arithmetic - and
the rule by which a set of rows is compared with it."""
import numpy as np

import profile_reference as pr

RTOL, COND_MAX, TIE_SHARE = pr.RTOL, pr.COND_MAX, pr.TIE_SHARE
FINE_FLOATS = ("kt_fine", "kt_lo_fine", "kt_hi_fine", "a_fine", "b_fine", "c0_fine", "sse_fine", "rmse_fine", "height_fine")
LEVELS = (1, 2)


def candidates(p, q):
    """x_l = p + (q - p) (l / 63) for l = 0..62 and x_63 = q: float64, one rounding per operation."""
    x = np.float64(p) + (np.float64(q) - np.float64(p)) * (np.arange(64, dtype=np.float64) / 63.0)
    x[63] = q
    return x


def _gap(v, thr):
    """The smallest relative distance of the sse values ``v`` from ``thr``: how close a decision against thr came."""
    v = np.asarray(v, dtype=np.float64)
    return float(np.min(np.abs(v - thr) / thr)) if v.size and thr > 0 else np.inf


def refine_cell(row, s, p, ages, R, delta, fit=pr.fit_age):
    """The fine fields of one fitted cell as a dict.  ``row``: the plain restatement's row (its 'curve' is the grid's sse),
    ``s`` and ``p``: the valid points.  Besides the fields: 'margin' (for the minimum, the lower and the upper end: how close
    the nearest decision on the way came to going the other way, relative) and 'cond' (the largest condition number of a
    candidate's design matrix; float64 lstsq alone)."""
    A, n, i = len(ages), row["n"], row["kt_index"]
    curve = np.asarray(row["curve"], dtype=np.float64)
    conds = [0.0]

    def fits(x):
        out = [fit(s, p, v) for v in x]
        if fit is pr.fit_age:
            conds.append(max(f[2] for f in out))
        sse = np.array([float(f[1]) for f in out])
        return out, sse

    best = dict(x=float(ages[i]), coef=(row["c0"], row["b"], row["a"]), sse=float(row["sse"]))
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
            best = dict(x=float(x[l]), coef=tuple(float(v) for v in out[l][0]), sse=float(sse[l]))
        else:
            margin[0] = min(margin[0], abs(best["sse"] - sse[l]) / best["sse"])
        thr = best["sse"] * (1.0 + delta / (n - 3))
        status = 0
        # the lower end
        g = int(np.flatnonzero(ages <= best["x"]).max())
        j = g
        while j >= 0 and curve[j] <= thr:
            j -= 1
        margin[1] = _gap(curve[max(j, 0):g + 1], thr)
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
                margin[1] = min(margin[1], _gap(sse[1:63], thr))
                pq = (x[l - 1], x[l])
            lo_x = float(pq[1])
        # the upper end
        g = int(np.flatnonzero(ages >= best["x"]).min())
        j = g
        while j <= A - 1 and curve[j] <= thr:
            j += 1
        margin[2] = _gap(curve[g:min(j, A - 1) + 1], thr)
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
                margin[2] = min(margin[2], _gap(sse[1:63], thr))
                pq = (x[l], x[l + 1])
            hi_x = float(pq[0])
    c0, b, a = (float(v) for v in best["coef"])
    return dict(kt_fine=best["x"], kt_lo_fine=lo_x, kt_hi_fine=hi_x, a_fine=a, b_fine=b, c0_fine=c0, sse_fine=best["sse"],
                rmse_fine=float(np.sqrt(best["sse"] / (n - 3))), height_fine=2.0 * a, status_fine=int(status), margin=margin,
                cond=max(conds))


def points_of(case, k):
    """(s, p) of the valid points of cell k of a case."""
    z, h = case["z"], case["h"]
    r, c = divmod(int(case["cells"][k]), z.shape[1])
    p = pr.sample_profile(z, float(r), float(c), np.sin(case["angle"][k]), np.cos(case["angle"][k]), h, case["w"])
    ok = ~np.isnan(p)
    return (np.arange(-h, h + 1).astype(np.float64) * case["de"])[ok], p[ok]


def restate(case, R, fit=pr.fit_age):
    """The rows of a case at R levels: the plain restatement's row of every cell (profile_reference.fit_cell), the fine
    fields and, where the cell is fitted, 's' and 'p' (its valid points)."""
    sa, ca = np.sin(case["angle"]), np.cos(case["angle"])
    rows = []
    for k in range(len(case["cells"])):
        row = pr.fit_cell(case["z"], case["de"], case["cells"][k], sa[k], ca[k], case["h"], case["w"], case["ages"],
                          case["delta"], case["min_samples"], fit=fit)
        if row["status"] == 1:
            row.update({f: np.nan for f in FINE_FLOATS}, status_fine=1, margin=[np.inf] * 3)
        else:
            s, p = points_of(case, k)
            fine = refine_cell(row, s, p, case["ages"], R, case["delta"], fit)
            fine["cond"] = max(fine["cond"], row["cond"])
            row.update(fine, s=s, p=p)
        rows.append(row)
    return rows


def compare(ref, got, case, R):
    """``got`` (per cell, anything indexable by the fine fields' names and n, status, sse) against ``ref`` (restate's rows in
    float64 lstsq).  Asserts what is exact or within RTOL, and returns the figures: cells, fitted, ties (cells where a pick
    parted that the restatement had decided within RTOL), the largest relative sse difference, the largest coefficient
    difference over the profile's range, the largest condition number."""
    h, de, delta = case["h"], case["de"], case["delta"]
    out = {"cells": len(ref), "fitted": 0, "ties": 0, "sse": 0.0, "coef": 0.0, "cond": 0.0}
    for r, g in zip(ref, got):
        cell = r["cell"]
        assert int(g["n"]) == r["n"] and (int(g["status"]) & 1) == (r["status"] & 1), cell
        if r["status"] == 1:
            assert int(g["status_fine"]) == 1 and all(np.isnan(float(g[f])) for f in FINE_FLOATS), cell
            continue
        out["fitted"] += 1
        assert r["cond"] <= COND_MAX, ("the inputs leave the tolerance's ground", cell, r["cond"])
        out["cond"] = max(out["cond"], r["cond"])
        fine = {f: float(g[f]) for f in FINE_FLOATS}
        n = r["n"]
        # structure: what the definition gives whatever was picked
        assert fine["kt_lo_fine"] <= fine["kt_fine"] <= fine["kt_hi_fine"], cell
        assert case["ages"][0] <= fine["kt_lo_fine"] and fine["kt_hi_fine"] <= case["ages"][-1], cell
        assert fine["sse_fine"] <= float(g["sse"]), cell
        assert fine["rmse_fine"] == float(np.sqrt(np.float64(fine["sse_fine"]) / (n - 3))), cell
        assert fine["height_fine"] == 2.0 * fine["a_fine"], cell
        # sse_fine and the coefficients against float64 lstsq at the age that was picked, unconditionally
        coef, sse, cond = pr.fit_age(r["s"], r["p"], fine["kt_fine"])
        assert cond <= COND_MAX, cell
        ds = abs(fine["sse_fine"] - sse) / sse
        dc = max(abs(fine["c0_fine"] - coef[0]), abs(fine["b_fine"] - coef[1]) * h * de, abs(fine["a_fine"] - coef[2])) / r["ptp"]
        assert ds <= RTOL, (cell, "sse_fine", ds)
        assert dc <= RTOL, (cell, "coefficients", dc)
        out["sse"], out["coef"] = max(out["sse"], ds), max(out["coef"], dc)
        # the picks: bit-equal, or parted where the restatement's own decision lay within RTOL
        tie = False
        if fine["kt_fine"] != r["kt_fine"]:
            assert r["margin"][0] <= RTOL, (cell, "kt_fine", fine["kt_fine"], r["kt_fine"], r["margin"])
            tie = True
        else:
            for e, f in ((1, "kt_lo_fine"), (2, "kt_hi_fine")):
                if fine[f] != r[f]:
                    assert r["margin"][e] <= RTOL, (cell, f, fine[f], r[f], r["margin"])
                    tie = True
        if tie:
            out["ties"] += 1
        else:
            assert int(g["status_fine"]) == r["status_fine"], (cell, g["status_fine"], r["status_fine"])
    assert out["ties"] <= TIE_SHARE * max(1, out["cells"]), out
    return out


# ---- the inputs of tests/test_gpu_refine.py (and of the two-arithmetics test on the CPU) ------------------------------------
def cut_to_the_cap(case):
    """The case with its age grid ended where the column-scaled condition number of a whole profile passes COND_MAX (at
    h = 15 the oldest ages are all but a line over the profile), as the plain fits' tests end theirs."""
    s = np.arange(-case["h"], case["h"] + 1).astype(np.float64) * case["de"]
    keep = [kt for kt in case["ages"] if pr.fit_age(s, s, kt)[2] <= COND_MAX]
    return dict(case, ages=np.asarray(keep, dtype=np.float64))


def line_cells(n, theta, rows):
    """The cells on the scarp's line of synthetic_scarp(n, theta=theta) in ``rows``, as segment_reference.noisy_case."""
    x = np.linspace(-n / 2, n / 2, num=n)
    yrot = -x[None, :] * np.cos(theta) + x[rows][:, None] * np.sin(theta)
    return rows.astype(np.int64) * n + np.argmin(np.abs(yrot), axis=1)


NAMES = ["synthetic h100 w2", "synthetic h15 w0", "h2", "one age", "64 ages", "best age below the grid",
         "best age above the grid", "borders, corners and NaN cells", "repeated cells", "no cell", "h1024"]

_CASES = []


def gpu_cases():
    """The cases as dicts (profile_reference.gpu_cases's keys), by NAMES.  Seeded and built once."""
    if _CASES:
        return _CASES
    from scarplet_amd import _plan
    ages = _plan.age_grid()
    rng = np.random.default_rng(20261020)

    def add(name, z, de, cells, angle, h, w, kt=ages, delta=1.0, ms=4):
        cells = np.ascontiguousarray(cells, dtype=np.int64)
        angle = np.ascontiguousarray(np.broadcast_to(np.asarray(angle, dtype=np.float64), cells.shape))
        _CASES.append(dict(name=name, z=z, de=float(de), cells=cells, angle=angle, h=h, w=w,
                           ages=np.asarray(kt, dtype=np.float64), delta=delta, min_samples=ms, sample=None))

    z = pr.synthetic_z(600)
    on = pr.scarp_cells(600, 100, rng, spread=3.0)
    ang = 0.2 + 0.05 * rng.standard_normal(100)
    add("synthetic h100 w2", z, 1.0, on, ang, 100, 2, ms=15)
    add("synthetic h15 w0", z, 1.0, on[:24], ang[:24], 15, 0, ms=12)
    _CASES[-1] = cut_to_the_cap(_CASES[-1])
    # five points, symmetric about j = 0: s and the erf of ANY age span their odd part, so every age gives the same sse and
    # the choice among candidates is rounding - with one age the bracket is a point, and the tie rule is all there is
    add("h2", z, 1.0, pr.scarp_cells(600, 40, rng, spread=1.0), 0.2, 2, 1, kt=ages[:1], ms=2)
    add("one age", z, 1.0, on[:16], ang[:16], 100, 2, kt=[10.0], ms=15)
    add("64 ages", z, 1.0, on[:16], ang[:16], 100, 2, kt=10 ** np.linspace(0, 3.4, 64), ms=15)
    # the scarp is 10 old: grids that begin above it and end below it put the minimum on their first and last age
    add("best age below the grid", z, 1.0, on[:16], ang[:16], 100, 2, kt=ages[14:24], ms=15)
    add("best age above the grid", z, 1.0, on[:16], ang[:16], 100, 2, kt=ages[:7], ms=15)
    # Borders, corners and NaN cells, ON the scarp's line (off it the sse curve is flat to 1e-9 and every pick is rounding):
    # profiles cut short by the top and bottom rows, profiles with a block and scattered cells missing on one side - no
    # symmetry of the profile may be assumed - and, at the corners and the side columns, rows of status 1
    n = 300
    zb = pr.synthetic_z(n, seed=7).copy()
    zb[rng.random(zb.shape) < 0.004] = np.nan
    zb[140:160, 160:175] = np.nan
    rows = np.concatenate([np.arange(0, 7), np.arange(293, 300), np.arange(134, 166, 3), rng.integers(40, 120, 6)])
    edge = np.concatenate([np.array([0, n - 1, n * (n - 1), n * n - 1]), rng.integers(0, n, 3) * n, rng.integers(0, n, 3) * n + n - 1,
                           line_cells(n, 0.2, rows)])
    add("borders, corners and NaN cells", zb, 1.0, edge, 0.2 + 0.1 * rng.standard_normal(len(edge)), 40, 3, ms=15)
    add("repeated cells", z, 1.0, np.repeat(on[:4], 3)[::-1], 0.2, 100, 5, ms=15, delta=0.0)
    add("no cell", z, 1.0, on[:0], 0.2, 100, 5, ms=15)
    zz = pr.synthetic_z(2400)
    add("h1024", zz, 1.0, pr.scarp_cells(2400, 4, rng, spread=10.0), 0.2, 1024, 1, ms=100)
    assert [c["name"] for c in _CASES] == NAMES
    return _CASES


_REF = {}


def reference(name, R):
    """restate() of a case in float64 lstsq, computed once and shared: not to be changed by a test."""
    if (name, R) not in _REF:
        _REF[(name, R)] = restate(gpu_cases()[NAMES.index(name)], R)
    return _REF[(name, R)]


# ---- what it recovers (docs/profiles.md, "Continuous ages") -----------------------------------------------------------------
KT0 = 10 ** 1.05                                                           # halfway between two grid ages, in log


def recovery_case(sigma):
    """synthetic_scarp(600, theta=0.2, kt0=KT0) with noise ``sigma`` and the 100 cells on its line of
    segment_reference.noisy_case; h = 100, w = 2."""
    from scarplet_amd import _plan
    z = pr.synthetic_z(600, theta=0.2, kt0=KT0, sigma=sigma)
    cells = line_cells(600, 0.2, np.arange(150, 450, 3))
    return dict(name="recovery, sigma %g" % sigma, z=z, de=1.0, cells=cells, angle=np.full(len(cells), 0.2), h=100, w=2,
                ages=_plan.age_grid(), delta=1.0, min_samples=15, sample=None)


def recovery_figures(rows, ages):
    """(median, largest |kt_fine / KT0 - 1|; the same of the grid's kt; the share of cells whose fine interval holds KT0)."""
    fine = np.array([abs(r["kt_fine"] / KT0 - 1.0) for r in rows])
    grid = np.array([abs(r["kt"] / KT0 - 1.0) for r in rows])
    holds = np.mean([r["kt_lo_fine"] <= KT0 <= r["kt_hi_fine"] for r in rows])
    return dict(fine_median=float(np.median(fine)), fine_max=float(fine.max()), grid_median=float(np.median(grid)),
                grid_max=float(grid.max()), holds=float(holds))
