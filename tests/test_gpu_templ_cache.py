"""Template coefficient planes kept across searches (sc_set_option "templ_gb", scarplet_amd/csrc/sc_templ_cache.h).

ONE check for every case: the record (sc_get_best: amp, snr, id) and - in exact mode - the result planes are identical
in every bit across three runs: a context with the cache off, the first search of a context with the cache on (all
misses) and the same search again (all hits, by sc_templ_cache_info).  The cases name a kernel class of the inverse
column pass each (the planes are read there), a launch form, a template family or a grid; then the rules of the key,
the budget, the allocation-pressure path, the templates the cache leaves alone, and two ranks on one GPU."""
import os
import sys

import numpy as np
import pytest

import scarplet_amd as sl
import scarplet_amd.dist as sd
from scarplet_amd import _lib, _plan, synthetic
from scarplet_amd import WindowedTemplate as WT
from tile_plans import forced_plan

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGES = [2.0, 10.0, 50.0]
FREQS = [0.05, 0.1, 0.2]
ANGLES = np.linspace(-1.2, 1.2, 5)
_DEMS = {}


def dem(key):
    """(n, ny, seed, de) -> DEMGrid, made once."""
    if key not in _DEMS:
        n, ny, seed, de = key
        _DEMS[key] = synthetic.synthetic_scarp(n, seed=seed, ny=ny, de=de)
    return _DEMS[key]


SMALL = (131, 150, 11, 1.0)          # 150 x 131: even ny, odd nx


def context(templ_gb, **options):
    ctx = _lib.Context(0)
    ctx.set_option("templ_gb", templ_gb)
    for k, v in options.items():
        ctx.set_option(k, v)
    return ctx


def same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), int((x != y).sum())


def natural(Template, scale, params, angles, **kw):
    """The search as Matcher.search plans it; exact: the float64 settle of its near-ties and the result planes."""
    def job(m, exact):
        m.search(Template, scale, params, angles, method="fft", exact=exact, **kw)
        assert m.method_used == "fft"
        out = [a.copy() for a in m.ctx.get_best()]
        if exact:
            assert m.exact_stats.get("route") == "device", m.exact_stats
            out.append(np.array(m.result_array()))
        return out
    return job


def forced(Template, scale, params, angles, Ty, Tx, nty=None, ntx=None):
    """The same through a hand-built tile plan (tests/tile_plans.py): any tile class on a small DEM."""
    def job(m, exact):
        par, ang = np.asarray(params, float), np.asarray(angles, float)
        arr, bbox, _ = m.describe(Template, scale, par, ang)
        sp = _lib.sc_plan(**forced_plan(m.ny, m.nx, bbox, Ty, Tx, nty, ntx, group=len(par)))
        if exact:
            assert m.can_flag_near_ties(arr, sp)
            m.run_described(arr, sp, m.exact_window_for(arr, sp), m.end_twins(arr, len(par), ang))
        else:
            m.run_described(arr, sp)
        out = [a.copy() for a in m.ctx.get_best()]
        if exact:
            out.append(np.array(m.ctx.get_result(np.repeat(par, len(ang)), np.tile(ang, len(par)))))
        return out
    return job


def rise(ctx, fn):
    """(what fn returns, the rise of the cache's counters while it ran, the counters after)"""
    before = ctx.templ_cache_info()
    out = fn()
    after = ctx.templ_cache_info()
    return out, {k: after[k] - before[k] for k in ("hits", "misses", "evictions")}, after


def three_runs(grid, job, exact, **options):
    """The check every case shares.  Returns the counters after the second search and the orientation runs it held."""
    off = context(0, **options)
    on = context(_lib.TEMPL_GB_AUTO, **options)
    try:
        cold = job(sl.Matcher(grid, ctx=off), exact)
        assert off.templ_cache_info() == dict(hits=0, misses=0, entries=0, bytes=0, evictions=0)
        m = sl.Matcher(grid, ctx=on)
        first, r1, i1 = rise(on, lambda: job(m, exact))
        assert r1["hits"] == 0 and r1["misses"] > 0 and r1["evictions"] == 0, r1            # all misses
        assert 0 < i1["entries"] <= r1["misses"] and i1["bytes"] > 0, i1
        second, r2, i2 = rise(on, lambda: job(m, exact))
        assert r2 == dict(hits=r1["misses"], misses=0, evictions=0), (r1, r2)                 # all hits
        assert (i2["entries"], i2["bytes"]) == (i1["entries"], i1["bytes"])
        same_bits(cold, first)
        same_bits(cold, second)
        assert (cold[1] > 0).any()
        return i2, r1["misses"]
    finally:
        off.close()
        on.close()


# name -> (DEM, job, what the counters must show: entries, runs)
CASES = {
    # ---- tile classes (the column kernel that reads the planes), on the 150 x 131 DEM
    "512 tiles (k_inv_cols_h2)": (SMALL, forced(WT.Scarp, 12, AGES, ANGLES, 512, 512, nty=2), None),
    "1024 tiles (k_inv_cols_w8), Ricker": (SMALL, forced(WT.Ricker, 8, [1.0, 2.0, 4.0], ANGLES, 1024, 1024, nty=2), None),
    "2048 tiles (k_inv_cols_w8)": (SMALL, forced(WT.Scarp, 12, AGES, ANGLES, 2048, 2048, nty=2), None),
    "one 2048 tile (paired templates, k_inv_cols_w4)": (SMALL, forced(WT.Scarp, 12, AGES, ANGLES, 2048, 2048), None),
    "three 512 tiles (a pair and the odd one)": (SMALL, forced(WT.Scarp, 12, AGES, ANGLES, 512, 512, nty=3), None),
    # ... and one orientation per launch sequence, the form of the large searches (an entry per run): the wave-per-column
    # kernel with two tile pairs interleaved, the paired templates of the odd tile
    "2048 tiles, two pairs, no batching": (SMALL, forced(WT.Scarp, 12, AGES, ANGLES, 2048, 2048, nty=2, ntx=2),
                                           lambda entries, runs: runs == 5 and entries == 5, dict(batch=0)),
    "three 1024 tiles, no batching": (SMALL, forced(WT.Ricker, 8, [1.0, 2.0, 4.0], ANGLES, 1024, 1024, nty=3),
                                      lambda entries, runs: runs == 5 and entries == 5, dict(batch=0)),
    # ---- launch forms and templates: a batched launch on a one-tile DEM holds several runs in one entry
    "batched orientations, Scarp": ((80, 96, 5, 1.0), natural(WT.Scarp, 10, [1.0, 10.0, 31.6], _plan.angle_grid(-0.035, 0.035)),
                                    lambda entries, runs: runs == 5 and entries < runs),
    "batched orientations, Channel": ((80, 96, 5, 1.0), natural(WT.Channel, 8, FREQS, _plan.angle_grid(-0.035, 0.035)),
                                      lambda entries, runs: runs == 5 and entries < runs),
    # ---- grids: one 2048 x 2048 tile with 3 ages x 5 orientations; odd extents (the parity key)
    "2048 x 2048, 3 ages x 5 orientations": ((2048, 2048, 3, 1.0), natural(WT.Scarp, 20, [5.0, 10.0, 20.0], ANGLES), None),
    "600 x 500": ((500, 600, 7, 1.0), natural(WT.Scarp, 14, AGES, ANGLES), None),
    "700 x 901, Channel": ((901, 700, 8, 2.0), natural(WT.Channel, 16, FREQS, ANGLES), None),
}


@pytest.mark.parametrize("exact", (False, True), ids=("float32", "exact"))
@pytest.mark.parametrize("name", list(CASES))
def test_cold_first_and_repeated_search_give_the_same_bits(name, exact):
    key, job, shows = CASES[name][:3]
    info, runs = three_runs(dem(key), job, exact, **(CASES[name][3] if len(CASES[name]) > 3 else {}))
    print("%s, %s: %d runs in %d entries, %.1f MB" % (name, "exact" if exact else "float32", runs, info["entries"],
                                                       info["bytes"] / 1e6))
    if shows is not None:
        assert shows(info["entries"], runs), (info, runs)


def test_batching_off_is_one_entry_per_run():
    info, runs = three_runs(dem((500, 600, 7, 1.0)), natural(WT.Scarp, 14, AGES, ANGLES), False, batch=0)
    assert runs == len(ANGLES) and info["entries"] == runs


def test_match_template_is_served_from_the_cache():
    """sc_match_template: one template, its maps."""
    g = dem(SMALL)
    off, on = context(0), context(_lib.TEMPL_GB_AUTO)
    try:
        maps = []
        for ctx in (off, on, on):
            m = sl.Matcher(g, ctx=ctx)
            arr, bbox, _ = m.describe(WT.Scarp, 12, np.asarray([10.0]), np.asarray([0.3]))
            sp = _lib.sc_plan(**forced_plan(m.ny, m.nx, bbox, 1024, 1024, group=1))
            maps.append([a.copy() for a in ctx.match_template(arr[0], sp)])
        assert on.templ_cache_info()["hits"] == 1 and on.templ_cache_info()["misses"] == 1
        same_bits(maps[0], maps[1])
        same_bits(maps[0], maps[2])
    finally:
        off.close()
        on.close()


def fresh(grid, job, exact=False, **options):
    ctx = context(0, **options)
    try:
        return job(sl.Matcher(grid, ctx=ctx), exact)
    finally:
        ctx.close()


def test_a_second_dem_of_the_same_shape_finds_every_entry():
    """Other values, same shape and spacing, on the same context: sc_set_dem does not clear the cache."""
    job = natural(WT.Scarp, 14, AGES, ANGLES)
    a, b = dem((500, 600, 7, 1.0)), dem((500, 600, 21, 1.0))
    on = context(_lib.TEMPL_GB_AUTO)
    try:
        _, r1, _ = rise(on, lambda: job(sl.Matcher(a, ctx=on), False))
        for exact in (False, True):
            out, r2, _ = rise(on, lambda: job(sl.Matcher(b, ctx=on), exact))
            assert r2 == dict(hits=r1["misses"], misses=0, evictions=0), (exact, r1, r2)
            same_bits(out, fresh(b, job, exact))
        on.forget_spectra()                                    # ... nor does forget_spectra
        _, r3, _ = rise(on, lambda: job(sl.Matcher(b, ctx=on), False))
        assert r3["misses"] == 0 and r3["hits"] == r1["misses"]
        on.forget_templates()                                  # sc_forget_templates does
        assert on.templ_cache_info()["entries"] == 0 and on.templ_cache_info()["bytes"] == 0
        out, r4, _ = rise(on, lambda: job(sl.Matcher(b, ctx=on), False))
        assert r4["hits"] == 0 and r4["misses"] == r1["misses"]
        same_bits(out, fresh(b, job))
    finally:
        on.close()


def test_one_field_changed_misses_the_runs_it_touches():
    """Spacing, scale, one age and the DEM's row parity reach every run of the search; one orientation reaches its own
    run alone (batching off: an entry per run).  The changed search equals a fresh context's in every bit."""
    base = (500, 600, 7, 1.0)
    changed = {
        "spacing": ((500, 600, 7, 2.0), natural(WT.Scarp, 14, AGES, ANGLES), len(ANGLES)),
        "scale": (base, natural(WT.Scarp, 18, AGES, ANGLES), len(ANGLES)),
        "one age": (base, natural(WT.Scarp, 14, [2.0, 11.0, 50.0], ANGLES), len(ANGLES)),
        "row parity": ((500, 601, 7, 1.0), natural(WT.Scarp, 14, AGES, ANGLES), len(ANGLES)),
        "one orientation": (base, natural(WT.Scarp, 14, AGES, np.concatenate([ANGLES[:2], [0.05], ANGLES[3:]])), 1),
        "kind": (base, natural(WT.Channel, 14, FREQS, ANGLES), len(ANGLES)),
    }
    for what, (key, job, want_misses) in changed.items():
        on = context(_lib.TEMPL_GB_AUTO, batch=0)
        try:
            _, r0, _ = rise(on, lambda: natural(WT.Scarp, 14, AGES, ANGLES)(sl.Matcher(dem(base), ctx=on), False))
            assert r0["misses"] == len(ANGLES) and r0["hits"] == 0
            out, r1, _ = rise(on, lambda: job(sl.Matcher(dem(key), ctx=on), False))
            assert r1["misses"] == want_misses and r1["hits"] == len(ANGLES) - want_misses, (what, r1)
            same_bits(out, fresh(dem(key), job, batch=0))
        finally:
            on.close()


def entry_bytes(m, Template, scale, params, angles):
    """Bytes of one run's entry on the matcher's natural plan: two real coefficient planes per template and 24 bytes."""
    arr, bbox, max_area = m.describe(Template, scale, np.asarray(params, float), np.asarray(angles, float))
    p, _ = m.plan_for(bbox, max_area, "fft", None, n_params=len(params))
    return len(params) * (2 * (p.Tx // 2 + 4) * p.Ty * 4 + 24)


def test_a_small_budget_keeps_what_fits():
    """Room for 2 of 5 runs: the search keeps the two it met first (it never evicts what it has used itself) and runs
    the chain for the rest - this time and the next; another search then takes the room, least recently used first."""
    g = dem((500, 600, 7, 1.0))
    job = natural(WT.Scarp, 14, AGES, ANGLES)
    cold = fresh(g, job, batch=0)
    on = context(_lib.TEMPL_GB_AUTO, batch=0)
    try:
        m = sl.Matcher(g, ctx=on)
        S = entry_bytes(m, WT.Scarp, 14, AGES, ANGLES)
        on.set_option("templ_gb", 2.5 * S / 1e9)
        out, r1, i1 = rise(on, lambda: job(m, False))
        assert r1 == dict(hits=0, misses=5, evictions=0) and i1["entries"] == 2 and i1["bytes"] == 2 * S, (r1, i1, S)
        same_bits(cold, out)
        for _ in range(2):
            out, r2, i2 = rise(on, lambda: job(m, False))
            assert r2 == dict(hits=2, misses=3, evictions=0) and i2["entries"] == 2, (r2, i2)
            same_bits(cold, out)
        other = natural(WT.Scarp, 14, AGES, ANGLES + 0.01)
        out, r3, i3 = rise(on, lambda: other(m, False))
        assert r3 == dict(hits=0, misses=5, evictions=2) and i3["entries"] == 2 and i3["bytes"] <= 2.5 * S, (r3, i3)
        same_bits(out, fresh(g, other, batch=0))
        on.set_option("templ_gb", 0)                           # off: what is held goes
        assert on.templ_cache_info()["entries"] == 0 and on.templ_cache_info()["bytes"] == 0
    finally:
        on.close()


def test_allocation_pressure_drops_entries_and_the_search_succeeds():
    """The test hook "test_mem_gb" bounds the context a little above what the first search left; the next search's hand-off
    buffers are given all tile pairs at once (option "y_gb") and need the memory the entries hold: sc_ensure drops
    entries and the search runs - the same bits as on a fresh context."""
    g = dem(SMALL)
    job = forced(WT.Scarp, 12, AGES, ANGLES, 1024, 1024, nty=2, ntx=2)
    on = context(100.0, batch=0, y_gb=0.001)
    try:
        m = sl.Matcher(g, ctx=on)
        _, r1, i1 = rise(on, lambda: job(m, False))
        assert r1 == dict(hits=0, misses=5, evictions=0) and i1["entries"] == 5
        held = on.device_bytes() + i1["bytes"]
        on.set_option("test_mem_gb", (held + 8e6) / 1e9)
        on.set_option("y_gb", 1.0)
        out, r2, i2 = rise(on, lambda: job(m, False))
        assert r2["evictions"] > 0 and r2["hits"] + r2["misses"] == 5, r2
        assert on.device_bytes() + i2["bytes"] <= held + 8e6
        same_bits(out, fresh(g, job, batch=0, y_gb=1.0))
    finally:
        on.close()


def test_generic_and_window_templates_leave_the_cache_alone():
    """Generic templates (the complex-spectrum route: a Shifted class) and caller-owned windows (craters) keep the
    uncached path: no counter moves, and the bytes are those of a context with the cache off."""
    g = dem((530, 520, 9, 1.0))
    shifted = natural(WT.ShiftedLeftFacingUpperBreakScarp, 12, [4.0], _plan.angle_grid()[::36], dx=3, dy=-2)

    def craters(m, exact):
        try:
            m.search_craters([6.0, 9.0], [10.0], method="fft", exact=False)
            return [a.copy() for a in m.ctx.get_best()]
        finally:
            m.ctx.clear_windows()
    for job in (shifted, craters):
        on = context(_lib.TEMPL_GB_AUTO)
        try:
            m = sl.Matcher(g, ctx=on)
            a = job(m, False)
            b = job(m, False)
            assert on.templ_cache_info() == dict(hits=0, misses=0, entries=0, bytes=0, evictions=0)
            cold = fresh(g, job)
            same_bits(cold, a)
            same_bits(cold, b)
        finally:
            on.clear_windows()
            on.close()


def test_orientation_matcher_two_ranks_on_one_gpu():
    """dist.OrientationMatcher, two ranks as threads with a context each (tools/thread_transport.py): every rank's
    second search is served from its own cache and the folded record equals the first's."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from thread_transport import run_ranks
    g = dem((230, 200, 4, 1.0))
    angles = _plan.angle_grid(-np.pi / 2, np.pi / 2)[::15]

    def rank_body(rank, transport):
        ctx = context(_lib.TEMPL_GB_AUTO)
        try:
            om = sd.OrientationMatcher(rank, 2, None, backend="host", transport=transport, matcher=sl.Matcher(g, ctx=ctx))
            recs, rises = [], []
            for _ in range(2):
                _, r, _ = rise(ctx, lambda: om.search(sl.Scarp, 14, [1.0, 4.0, 20.0], angles, method="fft"))
                recs.append([a.copy() for a in ctx.get_best()] + [np.array(om.result_array())])
                rises.append(r)
            return recs, rises
        finally:
            ctx.close()

    outs = run_ranks(2, rank_body)
    for recs, (r1, r2) in outs:
        assert r1["hits"] == 0 and r1["misses"] > 0, r1
        assert r2 == dict(hits=r1["misses"], misses=0, evictions=0), (r1, r2)
        same_bits(recs[0], recs[1])
    same_bits(outs[0][0][0], outs[1][0][0])                   # (the ranks end with the same record)
