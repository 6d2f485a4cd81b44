#!/usr/bin/env python3
"""Developer check: the bytes and the launches of a fixed list of small searches through sc_match and sc_match_template, as
SHA-256 lines - one per output plane of get_best() (or of the maps), and after every search the rise of every launch
counter (ctx.profile_get()).

The list: both methods with batching on and off (the cases of tests/test_gpu_match_plan.py: every rule of the launch plan);
match_template maps on both paths; kept spectra (one matcher, a second scale on the same tile plan); near-tie flags on
(the flag plane and the sorted events as well); a masked built-in (UpperBreak) and a generic plugin with per-cell masks;
windows the host uploads (a Shifted class); an odd tile count; the forced tile plans of tests/tile_plans.py (every tile
size on the diagonal, even and odd counts, each family of tests/test_gpu_tile_classes.py) and the real-space classes of
tests/direct_classes.py (--small: without its DEMs of more than two million cells).

Two libraries that plan and compute the same thing print the same lines: run it once per library (SCARPLET_HIP_LIB
selects one) and diff.  The hashes depend on the device and are not fixtures."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--small", action="store_true", help="without the large DEMs of tests/direct_classes.py and the 4096 tiles")
a = ap.parse_args()


class MaskedPlugin(object):
    """A generic plugin: a 21 x 15 window of weights that change sign, window limits that are no rectangle and an error
    mask over the left half - the host uploads the window and both per-cell masks."""

    def __init__(self, scale, age, alpha, nx, ny, de):
        self.age, self.alpha, self.nx, self.ny = age, alpha, nx, ny

    def template(self):
        W = np.zeros((self.ny, self.nx))
        cy, cx = self.ny // 2, self.nx // 2
        i, j = np.mgrid[-10:11, -7:8]
        W[cy - 10:cy + 11, cx - 7:cx + 8] = np.sin(0.4 * i * np.cos(self.alpha) + 0.3 * j * np.sin(self.alpha) + 0.1 * self.age) + 0.05
        return W

    def get_window_limits(self):
        m = np.zeros((self.ny, self.nx), dtype=bool)
        m[:12, :] = True
        m[20:30, 40:55] = True
        return m

    def get_err_mask(self):
        m = np.zeros((self.ny, self.nx), dtype=bool)
        m[:, :self.nx // 3] = True
        return m


def main():
    import direct_classes as dc
    import test_gpu_match_plan as tp
    import test_gpu_tile_classes as tc
    from tile_plans import SIZES, forced_plan, count_with_parity
    import scarplet_amd as sl
    from scarplet_amd import _lib, _plan
    from scarplet_amd import WindowedTemplate as WT
    print("# build id %s" % _lib.load().sc_build_id().decode(), file=sys.stderr, flush=True)
    total = dict(searches=0, planes=0)

    def emit(label, names, arrays):
        for name, arr in zip(names, arrays):
            arr = np.ascontiguousarray(arr)
            total["planes"] += 1
            print("%s | %s %s %s" % (label, name, arr.shape, hashlib.sha256(arr.tobytes()).hexdigest()), flush=True)

    def counted(ctx, label, before):
        after = ctx.profile_get()
        total["searches"] += 1
        print("%s | launches %s" % (label, " ".join("%s=%d" % (k, after[k][0] - before[k][0]) for k in _lib.K_NAMES)), flush=True)

    def search(ctx, label, arr, sp, maps=False):
        before = ctx.profile_get()
        if maps:
            for k in (0, len(arr) - 1):
                emit("%s template %d" % (label, k), ("amp", "snr"), ctx.match_template(arr[k], sp))
        else:
            ctx.reset_best()
            ctx.match(arr, sp, sync=True)
            emit(label, ("amp", "snr", "id"), ctx.get_best())
        counted(ctx, label, before)

    def fresh(opts=()):
        ctx = _lib.Context(0)
        for k, v in opts:
            ctx.set_option(k, v)
        ctx.profile(0)
        return ctx

    def done(ctx):
        ctx.clear_windows()
        ctx.close()

    # ---- every rule of the launch plan, batching on and off; the maps of the same descriptors
    for name, c in tp.CASES.items():
        for batch in (1, 0):
            ctx = fresh((("batch", batch),))
            m = sl.Matcher(sl.DEMGrid.from_array(tp.dem(c[0][0], c[0][1], 3), c[1]), ctx=ctx)
            arr, sp, _, _ = tp.planned(m, name, bool(batch))
            search(ctx, "plan | %s | batch %d" % (name, batch), arr, sp)
            if batch:
                search(ctx, "plan | %s | maps" % name, arr, sp, maps=True)
            done(ctx)

    # ---- kept spectra: one matcher, a second scale on the same tile plan finds the first one's curvature spectra
    ctx = fresh()
    m = sl.Matcher(sl.DEMGrid.from_array(tp.dem(512, 512, 4), 1.0), ctx=ctx)
    ages, angles = np.array([2.0, 8.0, 20.0]), _plan.angle_grid()[::12]
    plans = []
    for scale in (14, 20, 14):
        arr, bbox, area = m.describe(WT.Scarp, scale, ages, angles)
        _, sp = m.plan_for(bbox, area, "fft", None, n_params=len(ages))
        plans.append((sp.Ty, sp.Tx, sp.Vy, sp.Vx))
        search(ctx, "kept spectra | scale %d" % scale, arr, sp)
    print("kept spectra | tile plans %s" % (plans,), flush=True)
    done(ctx)

    # ---- near-tie flags on, both paths: the record, the flag plane, the events (sorted: their order is the device's)
    for method in ("fft", "direct"):
        ctx = fresh((("near_window", 6e-4),))
        m = sl.Matcher(sl.DEMGrid.from_array(tp.dem(300, 310, 5), 1.0), ctx=ctx)
        ages, angles = np.array([2.0, 5.0, 10.0, 20.0]), _plan.angle_grid()[::10]
        arr, bbox, area = m.describe(WT.Scarp, 12, ages, angles)
        _, sp = m.plan_for(bbox, area, method, None, n_params=len(ages))
        label = "near_window | %s" % method
        search(ctx, label, arr, sp)
        ev = ctx.near_events()
        ev = ev[np.lexsort(ev.T[::-1])] if ev is not None and len(ev) else np.zeros((0, 4), np.uint32)
        emit(label, ("near", "events"), (ctx.near_ties(), ev))
        done(ctx)

    # ---- masks and uploaded windows, both paths: a masked built-in, a generic plugin with per-cell masks, a Shifted class
    for method in ("fft", "direct"):
        for label, cls, scale, params, kw in (("UpperBreak", WT.RightFacingUpperBreakScarp, 12, [3.0, 30.0], {}),
                                              ("generic plugin with masks", MaskedPlugin, 1, [1.0, 2.0], {}),
                                              ("Shifted (uploaded windows)", WT.ShiftedLeftFacingUpperBreakScarp, 10, [4.0, 9.0], dict(dx=3, dy=-2))):
            ctx = fresh()
            m = sl.Matcher(sl.DEMGrid.from_array(tp.dem(260, 270, 6), 1.0), ctx=ctx)
            angles = _plan.angle_grid()[::30]
            arr, bbox, area = m.describe(cls, scale, np.asarray(params), angles, **kw)
            _, sp = m.plan_for(bbox, area, method, None, n_params=len(params))
            search(ctx, "masks | %s | %s" % (label, method), arr, sp)
            search(ctx, "masks | %s | %s | maps" % (label, method), arr, sp, maps=True)
            done(ctx)

    # ---- the forced tile plans: every size on the diagonal, an even and an odd tile count, every family
    ctx = fresh()
    for family in tc.FAMILIES:
        g = tc.dem("A")
        m = sl.Matcher(g, ctx=ctx)
        arr, bbox = tc.described(m, family)
        span_y, span_x = bbox[1] - bbox[0], bbox[3] - bbox[2]
        for T in SIZES:
            if a.small and T == 4096:
                continue
            shapes = [(None, None), (count_with_parity(150, span_y, T, 2, odd=False), None),
                      (count_with_parity(150, span_y, T, 3, odd=True), count_with_parity(131, span_x, T, 1, odd=True))]
            for nty, ntx in shapes if T <= 2048 else shapes[:1]:
                f = forced_plan(m.ny, m.nx, bbox, T, T, nty, ntx, group=tc.GROUP)
                search(ctx, "tile plans | A %s T=%d %dx%d" % (family, T, f["nty"], f["ntx"]), arr, _lib.sc_plan(**f))
    done(ctx)

    # ---- the real-space classes
    for c in dc.CASES:
        ny, nx, _ = dc.DEMS[c["dem"]]
        if a.small and ny * nx > 2000000:
            continue
        ctx = fresh((("variant", c["variant"]), ("batch", 0 if c["batch_off"] else 1)))
        m = sl.Matcher(dc.dem(c["dem"]), ctx=ctx)
        arr, bbox, area = m.describe(dc.FAMILIES[c["family"]][0], c["scale"], np.asarray(c["params"], float), np.asarray(c["angles"], float))
        _, sp = m.plan_for(bbox, area, "direct", None, n_params=len(c["params"]))
        search(ctx, "direct classes | %s" % c["name"], arr, sp)
        done(ctx)
    print("# %d searches, %d planes" % (total["searches"], total["planes"]), flush=True)


if __name__ == "__main__":
    main()
