#!/usr/bin/env python3
"""Developer timing of sl.match_craters (docs/craters.md): --n x --n DEM (default 4096), --radii radii from 10 to 200
cells (default 20) x the 35 ages of the reference's grid.

  synthesis   device time of sc_crater_windows alone (the library's k_windows bracket around its two kernels)
  whole call  device time of every bracket of Matcher.search_craters, and its wall time with the result on the host
  host route  wall time of the same search with the windows evaluated by numpy on the host and sent through
              upload_window, one slot each - the route there was before the device made them.  The host side is
              written to be quick, not literal: per radius the cells between the ring's bounds are picked first and
              the strips' masks are shared by the 35 ages (the literal class, one full loop per template, takes
              minutes); its windows are checked against Crater.template()

Warm, median of --reps; the two routes alternate.  The condition: the whole call is faster than the host route."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--radii", type=int, default=20)
ap.add_argument("--rmax", type=float, default=200.0)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--method", default="auto")
a = ap.parse_args()


def host_windows(radii, ages, nx, ny, de):
    """Crater.template() over the support box of every (radius, age), radius-major."""
    from scarplet_amd import WindowedTemplate as WT
    t = WT.crater_tables(radii, ages, nx, ny, de)
    x, y = WT.centred_axis(nx, de), WT.centred_axis(ny, de)
    out = []
    for ib in range(len(radii)):
        pmin, pmax, qmin, qmax = (int(v) for v in t["boxes"][ib])
        X, Y = np.meshgrid(x[nx // 2 + qmin:nx // 2 + qmax + 1], y[ny // 2 + pmin:ny // 2 + pmax + 1])
        rho2 = X * X + Y * Y
        ii, jj = np.nonzero((rho2 >= t["ring"][ib, 0]) & (rho2 <= t["ring"][ib, 1]))
        xs, ys = X[ii, jj], Y[ii, jj]
        acc = np.zeros((len(ages), len(xs)))
        for k in range(len(t["theta_tab"])):
            ca, sa, sign = t["theta_tab"][k]
            xm, yp = xs - t["dxy"][ib, k, 0], ys + t["dxy"][ib, k, 1]
            xr = xm * ca + yp * sa
            sel = np.nonzero(abs(xr) < 1)[0]
            if not sel.size:
                continue
            yr = -xm[sel] * sa + yp[sel] * ca
            sel = sel[abs(yr) < t["d_half"]]
            if not sel.size:
                continue
            v = xr[sel]
            acc[:, sel] += sign * ((-v / t["age_tab"][:, :1]) * np.exp(-v ** 2. / t["age_tab"][:, 1:]))
        for ia in range(len(ages)):
            W = np.zeros(X.shape)
            W[ii, jj] = acc[ia]
            out.append(W)
    return out


def main():
    import scarplet_amd as sl
    from scarplet_amd import _plan, WindowedTemplate as WT
    rng = np.random.default_rng(3)
    z = (np.cumsum(rng.standard_normal((a.n, a.n)), 1) * 0.05 + rng.standard_normal((a.n, a.n)) * 0.03).astype(np.float32)
    radii = np.linspace(10.0, a.rmax, a.radii)
    ages = _plan.age_grid()
    m = sl.Matcher(sl.DEMGrid.from_array(z, 1.0))
    ctx = m.ctx
    tables = WT.crater_tables(radii, ages, a.n, a.n, 1.0)

    # the host route's windows are the class's
    wins = host_windows(radii[:2], ages[::17], a.n, a.n, 1.0)
    for k, (r, kt) in enumerate((r, kt) for r in radii[:2] for kt in ages[::17]):
        pmin, pmax, qmin, qmax = (int(v) for v in tables["boxes"][k // len(ages[::17])])
        ref = WT.Crater(r, kt, a.n, a.n, 1.0).template()[a.n // 2 + pmin:a.n // 2 + pmax + 1, a.n // 2 + qmin:a.n // 2 + qmax + 1]
        assert np.array_equal(ref != 0, wins[k] != 0) and np.abs(ref - wins[k]).max() <= 1e-13 * np.abs(ref).max()

    def total_ms():
        return sum(v[1] for v in ctx.profile_get().values())

    def device_route():
        m.search_craters(radii, ages, method=a.method, exact=False)
        return m.result_array()

    def host_route():
        m.search_craters(radii, ages, method=a.method, exact=False, host_windows=host_windows(radii, ages, a.n, a.n, 1.0))
        return m.result_array()

    res_d = np.array(device_route())                    # warm-up of both routes (buffers sized, plans made)
    method = m.method_used
    res_h = np.array(host_route())
    same = (res_d[1] == res_h[1]) & (res_d[2] == res_h[2])
    print("%d x %d DEM, %d radii %g..%g x %d ages = %d templates, %s path; support boxes %d..%d cells wide"
          % (a.n, a.n, len(radii), radii[0], radii[-1], len(ages), len(radii) * len(ages), method,
             tables["boxes"][0, 1] * 2 + 1, tables["boxes"][-1, 1] * 2 + 1))
    print("the two routes agree on (age, radius) in %d of %d cells; max |dSNR| / max SNR %.2e"
          % (int(same.sum()), same.size, np.abs(res_d[3] - res_h[3]).max() / res_d[3].max()))
    synth, dev, wall_d, wall_h, host_np = [], [], [], [], []
    ctx.profile(1)
    for _ in range(a.reps):
        ctx.clear_windows()
        ms0 = ctx.profile_get()["k_windows"][1]
        ctx.crater_windows(tables)
        synth.append(ctx.profile_get()["k_windows"][1] - ms0)
        ms0 = total_ms()
        t = time.perf_counter()
        device_route()
        wall_d.append(time.perf_counter() - t)
        dev.append(total_ms() - ms0)
        t = time.perf_counter()
        host_windows(radii, ages, a.n, a.n, 1.0)
        host_np.append(time.perf_counter() - t)
        t = time.perf_counter()
        host_route()
        wall_h.append(time.perf_counter() - t)
    ctx.profile(0)
    ctx.clear_windows()
    med = lambda v: float(np.median(v))
    print("synthesis (sc_crater_windows, 2 kernels): device %.3f ms (median of %d; min %.3f, max %.3f)"
          % (med(synth), a.reps, min(synth), max(synth)))
    print("whole call: device %.1f ms, of which the search %.1f ms and the synthesis %.2f %%; wall %.1f ms (min %.1f, max %.1f)"
          % (med(dev), med(dev) - med(synth), 100 * med(synth) / med(dev), 1e3 * med(wall_d), 1e3 * min(wall_d), 1e3 * max(wall_d)))
    print("host route (numpy windows + upload_window + the same search): wall %.1f ms (min %.1f, max %.1f), of which numpy %.1f ms"
          % (1e3 * med(wall_h), 1e3 * min(wall_h), 1e3 * max(wall_h), 1e3 * med(host_np)))
    ok = med(wall_d) < med(wall_h)
    print("match_craters / host route, end to end: %.3f%s" % (med(wall_d) / med(wall_h), "" if ok else " - MISSED"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
