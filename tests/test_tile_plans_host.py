"""tests/tile_plans.py - hand-built tile plans of any size and number on a small DEM - checked on the host: against
_plan.Plan's own geometry, for coverage, and through the numpy model of the kernels against the oracle."""
import numpy as np
import pytest

import scarplet_oracle as orc
import pipeline_model as pm
from scarplet_amd import _plan, WindowedTemplate as WT
from tile_plans import SIZES, ModelPlan, forced_plan, min_tiles, count_with_parity

BBOX = (-20, 19, -20, 20)          # Scarp, scale 12, ages 2 .. 50, orientations -1.2 .. 1.2 on a 150 x 131 DEM: spans 39 and 40


def _fields_of(p):
    return dict(method=1, Ty=p.Ty, Tx=p.Tx, Vy=p.Vy, Vx=p.Vx, nty=p.nty, ntx=p.ntx, circ_y=int(p.circ_y),
                circ_x=int(p.circ_x), Py=p.Py, Qx=p.Qx, group=1)


def test_model_plan_lays_tiles_out_as_the_planner_does():
    """ModelPlan.tiles() on a planner's own fields is Plan.tiles(): origins, valid extents, input windows."""
    for (ny, nx) in ((150, 131), (151, 130), (700, 700), (3001, 1234)):
        for t_max in SIZES:
            p = _plan.Plan(ny, nx, (0, ny, 0, nx), BBOX, t_max=t_max)
            assert ModelPlan(ny, nx, _fields_of(p)).tiles() == p.tiles()


@pytest.mark.parametrize("T", SIZES)
def test_forced_plan_against_the_planner(T):
    """Where the planner would choose the same (T, nt) the forced plan is the planner's: with one tile per axis
    (V enters only through min(V, n)) the same tiles; with several, on an axis the planner's tiles divide evenly
    (n = nt (T - span)), the same fields."""
    # (a small support makes the planner prefer 512-tiles to larger ones: from 2048 upwards a support that no smaller tile holds)
    h = 3 * T // 8
    bbox = BBOX if T <= 1024 else (-h, h - 1, -h, h)
    spy, spx = bbox[1] - bbox[0], bbox[3] - bbox[2]
    for nt in (1, 2, 3):
        ny, nx = nt * (T - spy) - (nt == 1), nt * (T - spx) - 2 * (nt == 1)       # (one tile: not the circular case)
        p = _plan.Plan(ny, nx, (0, ny, 0, nx), bbox, t_max=T)
        assert (p.Ty, p.Tx, p.nty, p.ntx) == (T, T, nt, nt) and not p.circ_y and not p.circ_x, p
        f = forced_plan(ny, nx, bbox, T, T, nt, nt)
        assert ModelPlan(ny, nx, f).tiles() == p.tiles()
        if nt > 1:
            assert f == _fields_of(p)
    # one tile of any size on a 150 x 131 DEM, T > n included: the planner's tile of that size would start there too
    # (64 and 128 need several tiles there: test_forced_plans_cover_the_dem checks their layout)
    f = forced_plan(150, 131, BBOX, T, T)
    assert (f["nty"] == f["ntx"] == 1) == (T >= 256)
    if T >= 256:
        assert ModelPlan(150, 131, f).tiles() == [(0, 0, 150, 131, 0 - BBOX[1], 1 - BBOX[3])]


@pytest.mark.parametrize("Ty", SIZES)
def test_forced_plans_cover_the_dem(Ty):
    """Smallest, even and odd tile counts on both DEM parities: V <= T - span (what sc_match checks of the templates), the tiles cover the DEM
    exactly once, none is empty; a count that cannot cover raises."""
    for (ny, nx, bbox) in ((150, 131, BBOX), (151, 130, (-19, 19, -20, 19)), (150, 131, (-21, 19, -20, 20))):
        spy, spx = bbox[1] - bbox[0], bbox[3] - bbox[2]
        for Tx in SIZES:
            counts = [(None, None), (count_with_parity(ny, spy, Ty, 2, False), None),
                      (count_with_parity(ny, spy, Ty, 3, True), count_with_parity(nx, spx, Tx, 1, True))]
            for nty, ntx in counts:
                f = forced_plan(ny, nx, bbox, Ty, Tx, nty, ntx)
                assert 1 <= f["Vy"] <= Ty - spy and 1 <= f["Vx"] <= Tx - spx
                assert (f["Py"], f["Qx"], f["circ_y"], f["circ_x"]) == (bbox[1], bbox[3], 0, 0)
                seen = np.zeros((ny, nx), int)
                for (i0, j0, vy, vx, gi0, gj0) in ModelPlan(ny, nx, f).tiles():
                    assert vy >= 1 and vx >= 1
                    assert (gi0, gj0) == (i0 + ny % 2 - bbox[1], j0 + nx % 2 - bbox[3])
                    seen[i0:i0 + vy, j0:j0 + vx] += 1
                assert (seen == 1).all()
                if nty is None:
                    assert (f["nty"], f["ntx"]) == (min_tiles(ny, spy, Ty), min_tiles(nx, spx, Tx))
    assert min_tiles(150, 39, 64) == 6 and min_tiles(131, 40, 64) == 6
    for bad in (dict(nty=2), dict(nty=5), dict(ntx=5)):
        with pytest.raises(ValueError):
            forced_plan(150, 131, BBOX, 64, 64, **bad)
    with pytest.raises(ValueError):
        forced_plan(150, 131, (-40, 40, -20, 20), 64, 64)          # (a support no 64-tile holds)
    with pytest.raises(ValueError):
        forced_plan(150, 131, BBOX, 96, 64)                        # (not a tile size)


MODEL_CASES = [
    # class, kind, (ny, nx), (Ty, Tx), (nty, ntx), support boxes widened by a row
    (WT.Scarp, orc.SCARP, (150, 131), (64, 128), (None, None), False),        # 7 x 2 tiles
    (WT.Scarp, orc.SCARP, (150, 131), (256, 512), (None, None), False),       # one tile, T > n on both axes
    (WT.Ricker, orc.RICKER, (151, 130), (512, 64), (2, None), False),         # T > n along y, two rows of tiles
    (WT.LeftFacingUpperBreakScarp, orc.LEFT_UPPER, (150, 131), (128, 256), (3, 1), True),
    (WT.Scarp, orc.SCARP, (150, 131), (4096, 64), (None, None), False),       # the largest tile along y, six tiles along x
    (WT.Ricker, orc.RICKER, (151, 130), (128, 4096), (None, None), False),    # ... and along x
]


@pytest.mark.parametrize("case", MODEL_CASES, ids=lambda c: "%s-%dx%d" % ((c[1],) + c[3]))
def test_forced_plans_through_the_numpy_model(case):
    """Forced plans - a tile larger than the DEM among them, and descriptors whose boxes are a row larger than the
    support (they no longer map onto themselves under the flip: the library's parity-0 path) - through the numpy model of the kernels against the oracle."""
    cls, kind, (ny, nx), (Ty, Tx), (nty, ntx), widen = case
    rng = np.random.default_rng(17)
    z = (np.cumsum(rng.standard_normal((ny, nx)), 1) * 0.05 + rng.standard_normal((ny, nx)) * 0.02).astype(np.float32)
    xa, ya = WT.centred_axis(nx, 1.0), WT.centred_axis(ny, 1.0)
    A, B, C = pm.curvature_planes(z, 1.0, 1.0)
    scale, params, ang = (8, [1.0, 4.0], -0.6) if kind == orc.RICKER else (12, [2.0, 50.0], 1.2)
    cc, sc2, ss = _plan.curvature_coefficients(ang)
    curv = cc * A - sc2 * B + ss * C
    descs = [cls(scale, p, ang, nx, ny, 1.0)._device_descriptor() for p in params]
    if widen:
        for d in descs:
            d["bbox"] = (d["bbox"][0] - 1,) + tuple(d["bbox"][1:])
    bbox = _plan.bbox_union([d["bbox"] for d in descs])
    plan = ModelPlan(ny, nx, forced_plan(ny, nx, bbox, Ty, Tx, nty, ntx))
    assert plan.Ty > ny or plan.nty * plan.ntx > 1
    for p, d, (amp, snr) in zip(params, descs, pm.match_batch_fft(curv, descs, plan, xa, ya)):
        o_amp, _, _, o_snr = orc.match_template(z, 1.0, 1.0, kind, scale, p, ang)
        assert np.allclose(amp, o_amp, rtol=1e-8, atol=1e-10)
        assert np.allclose(snr, o_snr, rtol=1e-6, atol=1e-8)


def test_the_planner_reaches_4096_on_its_own():
    """A 4096 x 4096 DEM with a support of about 1500 cells: eight 2048-tiles cost more than the circular 4096-tile,
    so the library's generic path at 4096 is what a user's search runs."""
    p = _plan.Plan(4096, 4096, (0, 4096, 0, 4096), (-750, 750, -750, 750))
    assert (p.Ty, p.Tx, p.nty, p.ntx) == (4096, 4096, 1, 1) and p.circ_y and p.circ_x
    # ... and without the DEM's own periodicity, on a DEM no smaller tile holds the support of
    q = _plan.Plan(5000, 5000, (0, 5000, 0, 5000), (-1100, 1100, -1100, 1100))
    assert (q.Ty, q.Tx) == (4096, 4096) and not q.circ_y and q.nty * q.ntx > 1
