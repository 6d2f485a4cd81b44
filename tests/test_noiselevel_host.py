"""Host side of the curvature noise estimate (scarplet_amd/noise.py): the Gaussian weights the
device is given and the per-orientation quadratic form, both without a GPU.

The golden fixture (tests/golden/ref_noiselevel.npz, tools/gen_noiselevel_golden.py) holds the
unmodified reference's _estimate_curvature_noiselevel (dem.py:152-179) on four grids; here the
moments come from scipy-filtered stencil planes instead of the device."""
import numpy as np
import pytest

import scarplet_oracle as orc
from conftest import golden
from scarplet_amd import noise
from scarplet_amd.dem import DEMGrid

SIGMAS = (0.3, 1.0, 1.5, 7, 37.2, 100, 100.0, 250)
CASES = ("gc", "carrizo", "gc_dy", "tiny")


def golden_case(name):
    """(z with its NaN cells, dx, dy, angles, mean, sd) of one case of ref_noiselevel.npz."""
    f = np.load(golden("ref_noiselevel.npz"), allow_pickle=False)
    dx, dy = f[name + "_d"]
    if name + "_z" in f.files:
        z = f[name + "_z"].copy()
    else:
        r0, r1, c0, c1 = f[name + "_slice"]
        z = np.load(golden(str(f[name + "_fixture"])))["z"][r0:r1, c0:c1].astype(float)
        for a, b, c, d in f[name + "_nan_boxes"]:
            z[a:b, c:d] = np.nan
    return z, float(dx), float(dy), f[name + "_angles"], f[name + "_mean"], f[name + "_sd"]


def scipy_moments(z, dx, dy, sigma):
    """The 20 numbers of sc_curvature_noise, restated with numpy and scipy: moments of
    P - gaussian_filter(P, sigma) over the zero-filled grid's stencil planes, over all cells
    and over the cells farther than the radius from every NaN cell."""
    ndimage = pytest.importorskip("scipy.ndimage")
    nan = np.isnan(z)
    z0 = np.where(nan, 0.0, z)
    H = np.stack([P - ndimage.gaussian_filter(P, sigma, mode="reflect")
                  for P in orc.curvature_components(z0, dx, dy)], axis=-1).reshape(-1, 3)
    r = int(4.0 * float(sigma) + 0.5)
    box = ndimage.maximum_filter(nan.astype(np.uint8), size=2 * r + 1, mode="constant").astype(bool)
    out = []
    for keep in (np.ones(z.size, bool), ~box.ravel()):
        h = H[keep]
        if h.shape[0] == 0:
            out.extend([0.0] * 10)
            continue
        mu = h.mean(axis=0)
        d = h - mu
        c = d.T @ d
        out.extend([float(h.shape[0])] + list(mu) + [c[0, 0], c[0, 1], c[0, 2], c[1, 1], c[1, 2], c[2, 2]])
    return np.array(out)


def compare(name, mean, sd, ref_mean, ref_sd):
    """Largest |d mean| and |d sd| relative to the largest reference sd; NaN where the reference has NaN."""
    mean, sd = np.asarray(mean, dtype=float), np.asarray(sd, dtype=float)
    ref_mean, ref_sd = np.asarray(ref_mean, dtype=float), np.asarray(ref_sd, dtype=float)
    assert np.array_equal(np.isnan(sd), np.isnan(ref_sd)), (name, np.flatnonzero(np.isnan(sd)),
                                                            np.flatnonzero(np.isnan(ref_sd)))
    assert np.array_equal(np.isnan(mean), np.isnan(ref_mean)), name
    ok = ~np.isnan(ref_sd)
    scale = np.max(ref_sd[ok]) if ok.any() else 0.0
    scale = scale if scale > 0 else 1.0                 # (a flat grid: every sd is 0)
    e_sd = np.max(np.abs(sd[ok] - ref_sd[ok])) / scale if ok.any() else 0.0
    e_mean = np.max(np.abs(mean[ok] - ref_mean[ok])) / scale if ok.any() else 0.0
    print("noiselevel %-28s worst |d sd| %.2e, |d mean| %.2e (x max sd %.3e), NaN at %s"
          % (name, e_sd, e_mean, scale, list(np.flatnonzero(~ok))))
    return e_sd, e_mean


@pytest.mark.parametrize("sigma", SIGMAS)
def test_weights_are_gaussian_filter1d_bit_for_bit(sigma):
    ndimage = pytest.importorskip("scipy.ndimage")
    w, r = noise.gaussian_weights(sigma)
    assert r == int(4.0 * float(sigma) + 0.5) and w.shape == (2 * r + 1,)
    impulse = np.zeros(4 * r + 3)
    impulse[2 * r + 1] = 1.0
    resp = ndimage.gaussian_filter1d(impulse, sigma, mode="constant")
    # the response to a unit impulse is the weights reversed (correlation), bit for bit
    assert np.array_equal(resp[r + 1:3 * r + 2][::-1], w)


@pytest.mark.parametrize("sigma", [0, -1.0, np.nan, np.inf, 1e7])
def test_weights_reject_bad_sigma(sigma):
    with pytest.raises(ValueError):
        noise.gaussian_weights(sigma)


@pytest.mark.parametrize("name", CASES)
def test_quadratic_form_reproduces_reference(name):
    z, dx, dy, angles, ref_mean, ref_sd = golden_case(name)
    mo = scipy_moments(z, dx, dy, 100)
    mean, sd = noise.noiselevel_from_moments(mo, angles, first_nan_clear=bool(np.isnan(z).any()))
    assert isinstance(mean, list) and isinstance(sd, list) and len(sd) == len(angles) == 180
    assert all(isinstance(v, float) for v in mean + sd)
    e_sd, e_mean = compare("host " + name, mean, sd, ref_mean, ref_sd)
    assert e_sd <= 1e-12 and e_mean <= 1e-12


def test_golden_cases_cover_nan_and_reflections():
    """The fixture exercises what it is meant to: NaN boxes (angle 0 differs or is NaN), and a
    grid smaller than the filter radius."""
    z, _, _, _, _, sd = golden_case("tiny")
    assert max(z.shape) < 400 and np.isnan(sd[0]) and not np.isnan(sd[1:]).any()
    z, _, _, _, _, sd = golden_case("gc")
    assert np.isnan(z).any() and not np.isnan(sd).any()


def test_empty_cell_set_gives_nan():
    mo = np.zeros(20)
    mo[:10] = [4, 1, 2, 3, 1, 0, 0, 1, 0, 1]
    mean, sd = noise.noiselevel_from_moments(mo, [0.0, 0.5], first_nan_clear=True)
    assert np.isnan(mean[0]) and np.isnan(sd[0])
    assert mean[1] == pytest.approx(np.cos(0.5) ** 2 * 1 - 2 * np.sin(0.5) * np.cos(0.5) * 2 + np.sin(0.5) ** 2 * 3)
    c, s = np.cos(0.5), np.sin(0.5)
    assert sd[1] == pytest.approx(np.sqrt((c ** 4 + 4 * s * s * c * c + s ** 4) / 4))


@pytest.mark.parametrize("shape", [(1, 1), (2, 40), (40, 2)])
def test_grids_below_3x3_are_refused(shape):
    """The device holds grids of at least 3 x 3 cells (sc_set_dem); smaller ones raise before any NaN is
    zero-filled."""
    z = np.ones(shape)
    z[0, 0] = np.nan
    g = DEMGrid.from_array(z, 1.0)
    with pytest.raises(ValueError):
        g._estimate_curvature_noiselevel()
