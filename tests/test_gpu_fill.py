"""The nodata fill (sc_fill_nodata: k_fill_scan, k_fill_idw, k_fill_smooth) on the MI355X at the shapes where it can
go wrong, bit for bit against the oracle's fill_nodata_pass: more than one block in x, searches that cross a block's
edge, distances 0, 1 / 2, 1, sqrt(2) (QUAD_CHECK's 2 < sqrt(2)**2) and far beyond the raster, the limit's refresh with
a quadrant missing, odd and even smoothing counts (the result ends in either ping-pong plane), grids of one row or
one column, a context whose buffers last held a larger grid, the driver loop - and grids with more rows than one
launch grid's y extent holds, for the fill, the curvature and a whole search.

Inputs are finite or NaN only: with infinities the oracle's count of NaN cells and the device's count of cells
without a source mean different things."""
import functools
import time

import numpy as np
import pytest

import scarplet_amd as sl
import scarplet_oracle as orc
from scarplet_amd import _lib
from test_gpu_parity import close_maps, grid

pytestmark = pytest.mark.gpu

PAIRS = [(0, 0), (0.5, 0), (1, 0), (np.sqrt(2), 0), (4, 0), (4.99, 1), (9, 3), (610, 2), (1e9, 0)]


def swath(ny=70, nx=600, seed=600):
    """Three blocks in x: speckle, holes across x = 256 and x = 512, dead columns 255 and 256, the first and last row
    and column dead (so all four corners are)."""
    rng = np.random.default_rng(seed)
    z = np.cumsum(rng.standard_normal((ny, nx)), 1) + 50.0
    z[rng.random(z.shape) < 0.03] = np.nan
    z[20:33, 250:262] = np.nan
    z[40:52, 505:520] = np.nan
    z[:, 255:257] = np.nan
    z[0] = z[-1] = np.nan
    z[:, 0] = z[:, -1] = np.nan
    return z


@functools.lru_cache(maxsize=None)
def oracle_pass(transposed, dist, smooth):
    z = swath()
    out = orc.fill_nodata_pass(np.ascontiguousarray(z.T) if transposed else z, dist, smooth)
    out.setflags(write=False)
    return out


def equals_oracle(ctx, z, dist, smooth, ref=None):
    mine = z.copy()
    left = ctx.fill_nodata(mine, dist, smooth)
    if ref is None:
        ref = orc.fill_nodata_pass(z, dist, smooth)
    assert np.array_equal(mine, ref, equal_nan=True), (z.shape, dist, smooth, int(np.sum(~(mine == ref) & ~np.isnan(ref))))
    assert left == int(np.isnan(ref).sum())
    return mine


@pytest.fixture(scope="module")
def ctx():
    return _lib.Context(0)


@pytest.mark.parametrize("dist, smooth", PAIRS)
def test_three_blocks_in_x(ctx, dist, smooth):
    z = swath()
    out = equals_oracle(ctx, z, dist, smooth, oracle_pass(False, dist, smooth))
    if dist < 1:
        assert np.array_equal(np.isnan(out), np.isnan(z))              # nothing lies within reach
    if dist >= 610:
        assert not np.isnan(out).any()


@pytest.mark.parametrize("dist, smooth", PAIRS)
def test_one_block_in_x_deep_in_y(ctx, dist, smooth):
    z = np.ascontiguousarray(swath().T)
    equals_oracle(ctx, z, dist, smooth, oracle_pass(True, dist, smooth))


@pytest.mark.parametrize("shape", [(1, 300), (300, 1), (2, 2), (1, 1)])
def test_degenerate_grids(ctx, shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    z = np.cumsum(rng.standard_normal(shape), 1) + 50.0
    z[shape[0] // 2, (2 * shape[1]) // 3] = np.nan
    for dist, smooth in ((0, 0), (0.5, 0), (1, 0), (np.sqrt(2), 1), (2.5, 2), (400, 1), (1e9, 0)):
        out = equals_oracle(ctx, z, dist, smooth)
        if shape == (1, 1):                                            # the one cell is the whole grid: left == 1
            assert np.isnan(out).all() and ctx.fill_nodata(z.copy(), dist, smooth) == 1
        elif dist >= 1:
            assert not np.isnan(out).any()


def test_every_smoothing_count_ends_in_the_right_plane(ctx):
    z = swath()
    outs = [equals_oracle(ctx, z, 9, k, oracle_pass(False, 9, k)) for k in range(5)]
    filled = np.isnan(z) & ~np.isnan(outs[0])
    assert filled.sum() > 1000
    for k in range(4):
        assert np.array_equal(np.isnan(outs[k]), np.isnan(outs[0]))
        assert (outs[k + 1][filled] != outs[k][filled]).any()          # a pass that did nothing would show here
        assert np.array_equal(outs[k + 1][~filled], outs[k][~filled], equal_nan=True)


def test_a_smaller_grid_after_a_larger_one():
    """The reused fill[] buffers and the smoothing plane carved from the up | down tables, with a stale tail."""
    c = _lib.Context(0)
    z = swath()
    equals_oracle(c, z, 9, 1, oracle_pass(False, 9, 1))
    small = np.ascontiguousarray(swath(30, 40, 41))
    for dist, smooth in ((3, 0), (3, 1), (3, 2), (50, 3)):
        equals_oracle(c, small, dist, smooth)
    equals_oracle(c, z, 9, 2, oracle_pass(False, 9, 2))


def test_the_driver_loop():
    z = swath()
    g = sl.DEMGrid.from_array(z.copy(), 1.0)
    g._fill_nodata()
    assert g.is_interpolated and np.array_equal(g.nodata_mask, np.isnan(z))
    assert np.array_equal(g._griddata, orc.fill_nodata(z))


# ------------------------------------------------------------------ more rows than gridDim.y holds
# k_fill_idw, k_fill_smooth, k_curv_planes and k_curv_f64 are launched with gridDim.y = the row count.  The runtime
# takes 70000 rows in y as it stands (measured: these tests pass on the unchanged launch code); they pin that.  The
# oracle's search of the 70000 x 64 DEM (23 orientations, float64 FFTs of the whole grid) is computed once for both
# methods and takes about 13 s of CPU time, far more than the device's 0.07 s.
LONG = 70000


def test_fill_with_more_rows_than_one_launch_grid(ctx):
    rng = np.random.default_rng(70000)
    z = np.cumsum(rng.standard_normal((LONG, 3)), 1) + 50.0
    z[30000:30040] = np.nan
    z[65530:65545, 1] = np.nan
    z[-1] = np.nan
    for dist in (1, 25):
        out = equals_oracle(ctx, z, dist, 1)
        assert not np.isnan(out[65530:65545]).any() and not np.isnan(out[-1]).any()
        assert np.isnan(out[30000:30040]).any() == (dist == 1)


@functools.lru_cache(maxsize=None)
def long_dem():
    rng = np.random.default_rng(64)
    z = np.cumsum(rng.standard_normal((LONG, 64)), 1)
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def long_oracle():
    t0 = time.perf_counter()
    out = orc.match(long_dem(), 1.0, 1.0, orc.SCARP, scale=10., age=10., ang_min=-0.2, ang_max=0.2)
    print("oracle search of %d x 64: %.1f s" % (LONG, time.perf_counter() - t0))
    return out


def test_curvature_with_more_rows_than_one_launch_grid():
    z = long_dem()
    got = grid(z.copy(), 1.5, 2.5)._calculate_directional_laplacian(0.3)
    assert np.array_equal(got, orc.directional_curvature(z, 1.5, 2.5, 0.3))


@pytest.mark.parametrize("method", ["direct", "fft"])
def test_search_with_more_rows_than_one_launch_grid(method):
    z = long_dem()
    res = np.asarray(sl.match(grid(z.copy(), 1.0), sl.Scarp, scale=10., age=10., ang_min=-0.2, ang_max=0.2, method=method))
    assert res.shape == (4, LONG, 64)
    ref = long_oracle()
    for rows in (slice(0, 5000), slice(65000, LONG)):
        ok, err = close_maps(res[0][rows], res[3][rows], ref[0][rows], ref[3][rows])
        assert ok, (method, rows, err)
        assert ref[3][rows].max() > 0
