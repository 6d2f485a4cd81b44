"""The plan is what runs: a search's launch counters (ctx.profile_get(): counted whether or not timing is on) rise by
what sc_match_plan's chunks predict - tests/match_plan_reference.py restates the plan and the launch shapes from the
descriptors of Matcher.describe and the tile plan of Matcher.plan_for.  k_windows: one launch per chunk on the FFT path,
two in real space (k_direct_prep counts there too); k_direct: one per chunk; k_inv_cols and k_inv_rows: summed over
chunks, tile-pair chunks, groups of templates and slices of orientations.

The cases are the smallest at which each rule of the plan acts, each with batching on and off."""
import numpy as np
import pytest

import match_plan_reference as mp
import scarplet_amd as sl
from scarplet_amd import _plan
from scarplet_amd import WindowedTemplate as WT

pytestmark = pytest.mark.gpu

COUNTERS = ("k_windows", "k_direct", "k_inv_cols", "k_inv_rows")


def dem(ny, nx, seed):
    rng = np.random.default_rng(seed)
    return (np.cumsum(rng.standard_normal((ny, nx)), 1) * 0.05 + rng.standard_normal((ny, nx)) * 0.03).astype(np.float32)


# name -> (DEM shape, cell size, class, scale, parameters, angles, method, what the plan must show with batching on)
CASES = {
    # the smoke search: 15 templates in one real-space launch sequence
    "real space, 3 ages x 5 orientations": ((96, 80), 1.0, WT.Scarp, 10, [1.0, 10.0, 31.6], _plan.angle_grid(-0.035, 0.035), "direct",
                                           lambda inp, p: [c.nb for c in p["chunks"]] == [5]),
    # one 512 tile, one template per orientation: 61 orientations ride in one launch sequence, in pairs on the odd tile
    "one 512 tile, one template per orientation": ((512, 512), 1.0, WT.Channel, 10., [0.1], _plan.angle_grid()[::3], "fft",
                                                   lambda inp, p: (inp.Ty, inp.Tx, inp.ntiles) == (512, 512, 1) and [c.nb for c in p["chunks"]] == [61]),
    # two tiles, three ages at nine orientations: one tile pair, a batch of whole orientations
    "two tiles, several ages": ((900, 505), 2.0, WT.Scarp, 100, [5.0, 10.0, 20.0], _plan.angle_grid(-0.07, 0.07), "fft",
                                lambda inp, p: inp.ntiles == 2 and len(p["chunks"]) == 1 and p["chunks"][0].nb == 9),
    # ten ages: six orientations fill the row pass's table - of 13, the last seven ride together; of 10, five and five
    "a tail that rides along": ((512, 512), 1.0, WT.Scarp, 20, list(np.linspace(2.0, 20.0, 10)), _plan.angle_grid()[::15][:13], "fft",
                                lambda inp, p: [c.nb for c in p["chunks"]] == [6, 7]),
    "a tail that is split evenly": ((512, 512), 1.0, WT.Scarp, 20, list(np.linspace(2.0, 20.0, 10)), _plan.angle_grid()[::18][:10], "fft",
                                    lambda inp, p: [c.nb for c in p["chunks"]] == [5, 5]),
    # 70 ages at two orientations: runs of 64 and 6, none alike its neighbour
    "more parameters than a group": ((400, 420), 1.0, WT.Scarp, 12, list(np.linspace(1.0, 30.0, 70)), [-0.4, 0.5], "fft",
                                     lambda inp, p: [(c.n, c.nb) for c in p["chunks"]] == [(64, 1), (6, 1)] * 2),
    # 300 orientations of one template, more than a launch sequence holds: full batches, and the last 108 split evenly
    "more templates than a batch": ((512, 512), 1.0, WT.Channel, 8., [0.2], np.linspace(-1.5, 1.5, 300), "fft",
                                    lambda inp, p: [c.nb for c in p["chunks"]] == [64, 64, 64, 54, 54]),
}


def planned(m, name, batch):
    """(descriptors, tile plan, In, the restated plan) of a case on the matcher ``m``."""
    _, _, cls, scale, params, angles, method, _ = CASES[name]
    arr, bbox, max_area = m.describe(cls, scale, np.asarray(params, float), np.asarray(angles, float))
    _, sp = m.plan_for(bbox, max_area, method, None, n_params=len(params))
    inp, templ = mp.of_search(m, arr, sp, batch_off=not batch)
    return arr, sp, inp, mp.plan(inp, templ)


@pytest.mark.parametrize("batch", (True, False), ids=("batch", "batch off"))
@pytest.mark.parametrize("name", list(CASES))
def test_the_counters_rise_by_what_the_plan_predicts(name, batch):
    shape, de = CASES[name][:2]
    ctx = sl._lib.Context(0)
    try:
        ctx.set_option("batch", 1 if batch else 0)
        m = sl.Matcher(sl.DEMGrid.from_array(dem(shape[0], shape[1], 3), de), ctx=ctx)
        arr, sp, inp, p = planned(m, name, batch)
        if batch:
            assert CASES[name][7](inp, p), (name, inp, [(c.n, c.nb) for c in p["chunks"]])        # the rule the case is here for acts
        else:
            assert all(c.nb == 1 for c in p["chunks"])
        want = mp.launches(inp, sp, p["chunks"])
        ctx.reset_best()
        before = ctx.profile_get()
        ctx.match(arr, sp, sync=True)
        after = ctx.profile_get()
        rise = {k: after[k][0] - before[k][0] for k in COUNTERS}
        assert rise == want, (name, rise, want, [(c.n, c.nb) for c in p["chunks"]])
        assert (ctx.get_best()[1] > 0).any()
    finally:
        ctx.clear_windows()
        ctx.close()
