"""The exact mode's routing in the three search drivers - Matcher.search, DistMatcher.search and
OrientationMatcher.search - side by side on the CPU: a context that records every call stands in for the device, and
each case checks the calls, in order, the path the search reports and its exact_stats."""
import warnings

import numpy as np
import pytest

from scarplet_amd import _plan, dist as sd, WindowedTemplate as WT
from scarplet_amd.core import Matcher

NY, NX = 300, 280
AGES = np.array([2.0, 30.0])
ANGLES = _plan.angle_grid(-np.pi / 2, np.pi / 2)[::30]        # both ends of the grid: two end twins for a Scarp
SETTLED = {"flagged_cells": 3, "changed_cells": 1, "float64_cells": 3, "max_f32_err": 1e-5}


class _Recorder(object):
    """The device as the drivers see it: every call is recorded; resolution_stats answers ``stats``."""

    def __init__(self, variant=0, stats=(100, 0)):
        self.calls, self.variant, self.stats = [], variant, stats
        self.masked_slots, self.device, self._slots = set(), 0, 0

    def set_option(self, name, value):
        self.calls.append(("set_option", name, float(value)))

    def reset_best(self):
        self.calls.append(("reset_best",))

    def match(self, templates, sp, sync=True):
        self.calls.append(("match", "fft" if sp.method == _plan.METHOD_FFT else "direct", len(templates)))

    def resolution_stats(self):
        self.calls.append(("resolution_stats",))
        return self.stats

    def settle_exact(self, n_twin, max_work):
        self.calls.append(("settle_exact", n_twin, max_work))
        return dict(SETTLED)

    def snapshot_best(self):
        self.calls.append(("snapshot_best",))

    def rank_candidates(self, fetch=True):
        self.calls.append(("rank_candidates",))
        return np.zeros((0, 2), np.uint32)

    def settle_pairs(self, templates, pairs, n_twin=0, max_work=0.0):
        self.calls.append(("settle_pairs", len(templates), n_twin, max_work))
        return dict(SETTLED)

    def upload_window(self, win):
        self.calls.append(("upload_window",))
        self._slots += 1
        return self._slots - 1

    def set_masks(self, slot, lim, err):
        self.calls.append(("set_masks", slot))
        self.masked_slots.add(slot)

    def set_dem(self, *a, **k):
        self.calls.append(("set_dem",))


class _MaskedPlugin(object):
    """A user plugin: the host uploads its window, which carries an error mask (only the real-space path flags it).
    HALF sets the window's size: 201 x 201 taps for 12 ages make the real-space search unaffordable, 21 x 21 do not."""
    HALF = 100

    def __init__(self, scale, age, alpha, nx, ny, de):
        self.age, self.alpha, self.nx, self.ny = age, alpha, nx, ny

    def template(self):
        W = np.zeros((self.ny, self.nx))
        h, cy, cx = self.HALF, self.ny // 2, self.nx // 2
        W[cy - h:cy + h + 1, cx - h:cx + h + 1] = self.age
        return W

    def get_window_limits(self):
        return np.zeros((self.ny, self.nx), dtype=bool)

    def get_err_mask(self):
        m = np.zeros((self.ny, self.nx), dtype=bool)
        m[:, :self.nx // 2] = True
        return m


class _SmallMaskedPlugin(_MaskedPlugin):
    HALF = 10


def _matcher(ctx, whole=True):
    m = object.__new__(Matcher)                          # host side only: descriptors and plans need no device
    m.ny, m.nx, m.de, m.core, m.whole = NY, NX, 1.0, (0, NY, 0, NX), whole
    m.dx = m.dy = 1.0
    m.ctx = ctx
    return m


def _run(driver, ctx, Template, params, angles, method, exact):
    """One search through ``driver``; returns (the calls after describe, method_used, exact_stats, warnings)."""
    scale = 1 if issubclass(Template, _MaskedPlugin) else 12
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        if driver == "matcher":
            m = d = _matcher(ctx)
            m.search(Template, scale, params, angles, method=method, exact=exact)
        elif driver == "dist":
            m = _matcher(ctx, whole=False)
            d = sd.DistMatcher(0, 1, (NY, NX), 1.0, 1.0, backend="host", matcher=m)
            d.search(Template, scale, params, angles, np.zeros((NY, NX)), method=method, exact=exact)
        else:
            m = _matcher(ctx)
            d = sd.OrientationMatcher(0, 1, None, backend="host", matcher=m)
            d.search(Template, scale, params, angles, method=method, exact=exact)
    stats = getattr(d, "exact_stats", None)
    calls = [c for c in ctx.calls if c[0] not in ("upload_window", "set_masks", "set_dem")]
    assert d.method_used == m.method_used
    return calls, d.method_used, stats, [str(w.message) for w in caught]


def _exact_calls(driver, path, window, n_templates, n_twin, replanned=False):
    """What an exact search that settles on the device sends, driver by driver."""
    nw = [("set_option", "near_window", window), ("match", path, n_templates)]
    if driver == "matcher":
        out = [("reset_best",)] + ([("reset_best",)] if replanned else []) + nw
        if path == "fft":
            out.append(("resolution_stats",))           # (method="fft": the warning's statistic)
        return out + [("set_option", "near_window", 0.0), ("settle_exact", n_twin, Matcher.EXACT_MAX_F64)]
    if driver == "dist":
        return [("reset_best",)] + nw + [("set_option", "near_window", 0.0),
                                         ("settle_exact", n_twin, Matcher.EXACT_MAX_F64)]
    return [("reset_best",)] + nw + [("set_option", "near_window", 0.0), ("snapshot_best",), ("rank_candidates",),
                                     ("settle_pairs", n_templates, n_twin, Matcher.EXACT_MAX_F64)]


def _settled_stats(driver, window):
    if driver == "matcher":
        return dict({"patches": 0}, **SETTLED, route="device", window=window)
    if driver == "dist":
        return SETTLED
    return dict(SETTLED, route="device, 1 ranks' candidates")


DRIVERS = ["matcher", "dist", "orientation"]


@pytest.mark.parametrize("driver", DRIVERS)
def test_builtin_scarp_settles_on_the_fft_tiles(driver):
    ctx = _Recorder()
    calls, used, st, msgs = _run(driver, ctx, WT.Scarp, AGES, ANGLES, "fft", True)
    n = len(AGES) * len(ANGLES)
    assert calls == _exact_calls(driver, "fft", 6e-4, n, len(AGES)), calls
    assert used == "fft" and st == _settled_stats(driver, 6e-4) and msgs == []


@pytest.mark.parametrize("driver", DRIVERS)
def test_builtin_scarp_is_exact_by_default(driver):
    ctx = _Recorder()
    calls, used, st, _ = _run(driver, ctx, WT.Scarp, AGES, ANGLES, "fft", None)
    assert calls == _exact_calls(driver, "fft", 6e-4, len(AGES) * len(ANGLES), len(AGES)), calls
    assert used == "fft" and st == _settled_stats(driver, 6e-4)


@pytest.mark.parametrize("driver", DRIVERS)
def test_upper_break_with_fft_is_replanned_onto_the_real_space_path(driver):
    ctx = _Recorder()
    calls, used, st, msgs = _run(driver, ctx, WT.LeftFacingUpperBreakScarp, AGES, ANGLES, "fft", True)
    n = len(AGES) * len(ANGLES)
    assert calls == _exact_calls(driver, "direct", 6.6e-4, n, 0, replanned=True), calls
    assert used == "direct" and st == _settled_stats(driver, 6.6e-4) and msgs == []


@pytest.mark.parametrize("driver", DRIVERS)
def test_variant_9_takes_the_real_space_path(driver):
    ctx = _Recorder(variant=9)
    calls, used, st, msgs = _run(driver, ctx, WT.Scarp, AGES, ANGLES, "fft", True)
    n = len(AGES) * len(ANGLES)
    assert calls == _exact_calls(driver, "direct", 6.6e-4, n, len(AGES), replanned=True), calls
    assert used == "direct" and st == _settled_stats(driver, 6.6e-4) and msgs == []


@pytest.mark.parametrize("driver", DRIVERS)
def test_masked_plugin_too_costly_for_the_real_space_path_keeps_float32(driver):
    ctx = _Recorder()
    ages = np.arange(1.0, 13.0)
    calls, used, st, msgs = _run(driver, ctx, _MaskedPlugin, ages, [0.2], "fft", True)
    assert used == "fft"
    if driver == "matcher":
        assert calls == [("reset_best",), ("set_option", "near_window", 0.0), ("match", "fft", 12),
                         ("set_option", "near_window", 0.0)], calls
        assert st["skipped"] is True and np.isnan(st["max_f32_err"])
        assert sorted(st) == sorted(["flagged_cells", "patches", "changed_cells", "float64_cells", "max_f32_err",
                                     "skipped"])
    else:
        want = [("reset_best",), ("match", "fft", 12)]
        assert calls == want, calls
        assert st == {"skipped": True}
    assert len(msgs) == 1 and msgs[0].startswith("exact=True: this plugin's templates carry per-cell masks"), msgs


@pytest.mark.parametrize("driver", DRIVERS)
def test_masked_plugin_within_reach_settles_on_the_real_space_path(driver):
    ctx = _Recorder()
    ages = np.array([1.0, 2.0, 3.0, 4.0])
    calls, used, st, msgs = _run(driver, ctx, _SmallMaskedPlugin, ages, [0.2], "fft", True)
    assert calls == _exact_calls(driver, "direct", 6.6e-4, 4, 0, replanned=True), calls
    assert used == "direct" and st == _settled_stats(driver, 6.6e-4) and msgs == []


@pytest.mark.parametrize("driver", DRIVERS)
def test_window_plugin_is_not_exact_by_default(driver):
    ctx = _Recorder()
    ages = np.array([1.0, 2.0, 3.0, 4.0])
    calls, used, st, msgs = _run(driver, ctx, _SmallMaskedPlugin, ages, [0.2], "fft", None)
    assert used == "fft" and not any(c[0] == "set_option" for c in calls)
    if driver == "matcher":
        assert calls == [("reset_best",), ("match", "fft", 4), ("resolution_stats",)], calls
        assert st is None
    else:
        assert calls == [("reset_best",), ("match", "fft", 4)], calls
        assert st is None
    assert msgs == []


def test_orientation_host_backend_without_transport_is_not_exact_by_default():
    ctx = _Recorder()
    m = _matcher(ctx)

    class _Transport(object):
        pass
    om = sd.OrientationMatcher(0, 2, None, backend="host", transport=_Transport(), matcher=m)
    om.transport = None
    seen = []
    om.run = lambda mine, sp, exact_window=0.0, n_twin=0: seen.append(exact_window)
    om.search(WT.Scarp, 12, AGES, ANGLES, method="fft")
    assert seen == [0.0] and om.method_used == "fft" and ctx.calls == []
    om.transport = _Transport()
    om.search(WT.Scarp, 12, AGES, ANGLES, method="fft")
    assert seen == [0.0, 6e-4]


def test_matcher_auto_reruns_an_unresolved_surface_on_the_real_space_path():
    n = len(AGES) * len(ANGLES)
    for exact in (False, True):
        ctx = _Recorder(stats=(100, 50))
        calls, used, st, msgs = _run("matcher", ctx, WT.Scarp, AGES, ANGLES, "auto", exact)
        if exact:
            want = [("reset_best",), ("set_option", "near_window", 6e-4), ("match", "fft", n), ("resolution_stats",),
                    ("reset_best",), ("set_option", "near_window", 6.6e-4), ("match", "direct", n),
                    ("set_option", "near_window", 0.0), ("settle_exact", len(AGES), Matcher.EXACT_MAX_F64)]
            assert st == _settled_stats("matcher", 6.6e-4)
        else:
            want = [("reset_best",), ("match", "fft", n), ("resolution_stats",), ("reset_best",), ("match", "direct", n)]
        assert calls == want, calls
        assert used == "direct"
        assert msgs == ["the FFT path cannot resolve 50.0 % of this surface's cells in float32 (no noise floor of its "
                        "own): searched again on the exact real-space path"], msgs
    # resolved: the FFT answer stands
    ctx = _Recorder(stats=(100, 1))
    calls, used, _, msgs = _run("matcher", ctx, WT.Scarp, AGES, ANGLES, "auto", False)
    assert calls == [("reset_best",), ("match", "fft", n), ("resolution_stats",)] and used == "fft" and msgs == []


def test_matcher_fft_only_warns_on_an_unresolved_surface():
    n = len(AGES) * len(ANGLES)
    for exact in (False, True):
        ctx = _Recorder(stats=(100, 50))
        calls, used, _, msgs = _run("matcher", ctx, WT.Scarp, AGES, ANGLES, "fft", exact)
        assert used == "fft"
        assert [c for c in calls if c[0] in ("match", "resolution_stats", "reset_best")] == \
            [("reset_best",), ("match", "fft", n), ("resolution_stats",)], calls
        assert len(msgs) == 1 and msgs[0].startswith("method='fft': 50.0 % of the cells this search won"), msgs


def test_matcher_unresolved_but_real_space_unaffordable_only_warns():
    ctx = _Recorder(stats=(100, 50))
    m = _matcher(ctx)
    m._direct_affordable = lambda bbox, max_area, n_par: False
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        m.search(WT.Scarp, 12, AGES, ANGLES, method="auto", exact=True)
    assert m.method_used == "fft" and [str(w.message) for w in caught] == [
        "the FFT path cannot resolve 50.0 % of this surface's cells in float32 (no noise floor of its own); "
        "method='direct' is exact but much slower here - not taken automatically"]
