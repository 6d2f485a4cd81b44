"""DEMGrid._estimate_curvature_noiselevel on the device (sc_curvature_noise) against the unmodified
reference (tests/golden/ref_noiselevel.npz) and against a restatement of dem.py:152-179 built
from the oracle's directional curvature and scipy's gaussian_filter.

Tolerance: |d sd| and |d mean| <= 1e-12 x the largest sd over the orientations; NaN at exactly the
reference's orientations.  Every comparison prints its worst error."""
import ctypes
import warnings

import numpy as np
import pytest

import scarplet_oracle as orc
import scarplet_amd as sl
from scarplet_amd import _lib
from scarplet_amd import WindowedTemplate as WT
from test_noiselevel_host import CASES, compare, golden_case

pytestmark = pytest.mark.gpu

TOL = 1e-12


class Grid(object):
    """A bare grid-like object (what `match` takes): _griddata and _georef_info only."""

    def __init__(self, z, dx, dy):
        self._griddata = z
        self._georef_info = type("GeorefInfo", (), {"dx": dx, "dy": dy})()


def restated(z, dx, dy, sigma, angles):
    """dem.py:152-179 literally: per orientation the curvature of the grid as it stands (the first
    call zero-fills the NaN cells in place), gaussian_filter, nanmean / nanstd of the high-pass."""
    ndimage = pytest.importorskip("scipy.ndimage")
    z = np.array(z, dtype=float)
    mean, sd = [], []
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # (nanmean / nanstd of an all-NaN orientation)
        for alpha in angles:
            del2z = orc.directional_curvature(z, dx, dy, alpha)
            z[np.isnan(z)] = 0
            hp = del2z - ndimage.gaussian_filter(del2z, sigma)
            mean.append(np.nanmean(hp))
            sd.append(np.nanstd(hp))
    return mean, sd


@pytest.mark.parametrize("name", CASES)
def test_golden_reference(name):
    z, dx, dy, angles, ref_mean, ref_sd = golden_case(name)
    nan = np.isnan(z)
    g = sl.DEMGrid.from_array(z, dx, dy)
    out_angles, mean, sd = g._estimate_curvature_noiselevel()
    assert isinstance(out_angles, np.ndarray) and np.array_equal(out_angles, angles)
    assert isinstance(mean, list) and isinstance(sd, list) and len(mean) == len(sd) == 180
    assert all(isinstance(v, float) for v in mean + sd)
    e_sd, e_mean = compare("device " + name, mean, sd, ref_mean, ref_sd)
    assert e_sd <= TOL and e_mean <= TOL
    # the reference's write-through: zeros where the grid held NaNs
    assert not np.isnan(g._griddata).any() and np.all(g._griddata[nan] == 0)
    assert np.array_equal(g._griddata[~nan], z[~nan])


SHAPES = [(3, 3), (3, 2000), (2000, 3), (37, 52), (64, 63), (301, 257)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("sigma", [1.5, 7, 100])
@pytest.mark.parametrize("with_nan", [False, True])
def test_restatement(shape, sigma, with_nan):
    ny, nx = shape
    rng = np.random.default_rng(ny * 7919 + nx * 31 + int(sigma * 10) + with_nan)
    z = np.cumsum(rng.standard_normal(shape), axis=1) * 0.7 + rng.standard_normal(shape) * 0.2 + 50.0
    if with_nan:
        z[rng.integers(ny), rng.integers(nx)] = np.nan
        if ny * nx > 4:
            z[rng.integers(ny), rng.integers(nx)] = np.nan
    dx, dy = 1.5, -0.8                                   # dx != |dy|
    angles = np.array([0.0, 0.3, np.pi / 4, 1.2, np.pi / 2, 2.5, np.pi])
    ref_mean, ref_sd = restated(z, dx, dy, sigma, angles)
    grid = Grid(z.copy(), dx, dy)
    a, mean, sd = sl.estimate_curvature_noiselevel(grid, sigma=sigma, angles=angles)
    assert np.array_equal(a, angles)
    e_sd, e_mean = compare("restated %dx%d s=%g nan=%d" % (ny, nx, sigma, with_nan), mean, sd, ref_mean, ref_sd)
    assert e_sd <= TOL and e_mean <= TOL
    assert not np.isnan(grid._griddata).any()


def test_same_bits_twice():
    z, dx, dy, _, _, _ = golden_case("gc")
    runs = []
    for _ in range(2):
        ctx = sl.core._context(0)
        zz = np.where(np.isnan(z), 0.0, z)
        ctx.set_dem(zz, dx, dy, WT.centred_axis(z.shape[1], dx), WT.centred_axis(z.shape[0], dx))
        w, _ = sl.noise.gaussian_weights(100)
        runs.append(ctx.curvature_noise(w, np.isnan(z)))
    assert runs[0].tobytes() == runs[1].tobytes()
    assert runs[0][0] == z.size and 0 < runs[0][10] < z.size
    a1 = sl.DEMGrid.from_array(z, dx, dy)._estimate_curvature_noiselevel()
    a2 = sl.DEMGrid.from_array(z, dx, dy)._estimate_curvature_noiselevel()
    assert np.array_equal(a1[1], a2[1]) and np.array_equal(a1[2], a2[2])


def test_block_context_and_bad_radius_are_invalid():
    ny, nx = 40, 50
    z = np.random.default_rng(3).standard_normal((ny + 4, nx + 4))
    ctx = _lib.Context(0)
    try:
        ctx.set_dem(z, 1.0, 1.0, WT.centred_axis(nx, 1.0), WT.centred_axis(ny, 1.0), origin=(-2, -2),
                    shape=(ny, nx), core=(0, ny, 0, nx), wrap=False)
        w = np.ones(3) / 3
        out = np.zeros(20)
        dp = ctypes.POINTER(ctypes.c_double)
        rc = ctx.lib.sc_curvature_noise(ctx._h, w.ctypes.data_as(dp), 1, None, out.ctypes.data_as(dp))
        assert rc == -1                                      # SC_ERR_INVALID
        ctx.set_dem(z, 1.0, 1.0, WT.centred_axis(nx + 4, 1.0), WT.centred_axis(ny + 4, 1.0))
        rc = ctx.lib.sc_curvature_noise(ctx._h, w.ctypes.data_as(dp), -1, None, out.ctypes.data_as(dp))
        assert rc == -1
        rc = ctx.lib.sc_curvature_noise(ctx._h, w.ctypes.data_as(dp), 1, None, out.ctypes.data_as(dp))
        assert rc == 0 and out[0] == z.size and np.array_equal(out[:10], out[10:])
    finally:
        ctx.close()
