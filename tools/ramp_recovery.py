#!/usr/bin/env python3
"""The 1-D figures of docs/profiles.md, "The initial slope" (CPU, the numpy restatement of tests/ramp_reference.py): what
the plain erf model, the model with the initial slope given and the model with the width free recover from profiles
z = a g(s; kt, L) + b s + noise with a = 1, b = -0.01, h = 100, de = 1, the default 35 ages, M = 8.  Seeded."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402


def main():
    import ramp_reference as rr
    from scarplet_amd import _plan
    ages = _plan.age_grid()
    h, de, M = 100, 1.0, 8
    j = np.arange(-h, h + 1)
    s = j * de
    E = rr.columns(j, h, M, de, ages, *rr._tables(h, M, de, ages))

    def run(L, idx, noise, count, seed):
        rng = np.random.default_rng(seed)
        out = {"plain": [], "given": [], "free": []}
        for _ in range(count):
            p = rr.g_exact(s, ages[idx], L) - 0.01 * s + noise * rng.standard_normal(len(s))
            coefs, grid = rr.fit_all_lstsq(s, p, E)
            pairs = dict(cell=0, n=len(s), usable=True, cond=0.0, ptp=1.0, grid=grid, coefs=coefs, slopes=rr.slopes_of(coefs, de))
            step = dict(pairs, grid=grid[:, :1], coefs=coefs[:, :1], slopes=pairs["slopes"][:, :1])
            out["plain"].append(rr.choose_cell(step, de, 0, ages))
            if L > 0:
                out["given"].append(rr.choose_cell(pairs, de, M, ages, rr.SLOPE, abs(-0.01 + 1.0 / L)))
            out["free"].append(rr.choose_cell(pairs, de, M, ages))
        return out

    width = lambda rows: float(np.mean([r["hi_index"] - r["lo_index"] + 1 for r in rows]))
    on = lambda rows, idx: sum(r["kt_index"] == idx for r in rows)
    for L, idx in ((6, 10), (4, 10), (8, 15)):
        for noise in (0.02, 0.05):
            r = run(L, idx, noise, 60, 0)
            print("L %d, true index %d, noise %.2f: plain model on index %d, the true age in %d of 60, mean interval %.2f ages; "
                  "slope given: the true age in %d of 60"
                  % (L, idx, noise, np.bincount([q["kt_index"] for q in r["plain"]]).argmax(), on(r["plain"], idx),
                     width(r["plain"]), on(r["given"], idx)))
    for L, idx in ((6, 10), (4, 10), (8, 15), (0, 10)):
        q = run(L, idx, 0.0, 1, 1)["free"][0]
        print("width free, no noise, L %d, true index %d: index %d, width_index %d" % (L, idx, q["kt_index"], q["width_index"]))
    for noise in (0.02, 0.05):
        r = run(6, 10, noise, 100, 1)
        print("width free, L 6, true index 10, noise %.2f: the true age in %d of 100, mean interval %.2f ages (plain: %.2f)"
              % (noise, on(r["free"], 10), width(r["free"]), width(r["plain"])))


if __name__ == "__main__":
    main()
