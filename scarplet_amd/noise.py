"""Noise level of the directional curvature (dem.py:152-179), computed on the device.

The reference's ``CalculationMixin._estimate_curvature_noiselevel`` computes, for each of 180
orientations, the directional curvature ``del2z``, its low-pass ``gaussian_filter(del2z, 100)``
(mode 'reflect') and ``nanmean`` / ``nanstd`` of the high-pass ``del2z - lowpass``.  Curvature
and filter are linear, so with the stencil planes A, B, C (d2z_dx2, d2z_dxdy, d2z_dy2) and
``H_P = P - G * P``::

    highpass(a) = c**2 H_A - 2 s c H_B + s**2 H_C        (c = cos a, s = sin a)
    mean(a) = v . mu,   var(a) = v' Sigma v,             v = (c**2, -2 s c, s**2)

with mu and Sigma the mean and covariance of (H_A, H_B, H_C).  The device filters the three
planes once and returns their moments (``sc_curvature_noise``); the host evaluates the
orientations (``noiselevel_from_moments``).

The reference's NaN handling is kept: its first orientation sees the NaN cells (later ones see
the grid its curvature call zero-filled, dem.py:84-86), and its filter spreads each NaN over a
(2 r + 1)^2 box that ``nanmean`` / ``nanstd`` drop.  So the first orientation counts only the
cells farther than r (Chebyshev distance) from every NaN cell - NaN when there are none - and
the others count every cell.
"""

import numpy as np

from scarplet_amd import _lib

TRUNCATE = 4.0      # gaussian_filter's default: the filter radius is int(4 sigma + 0.5)


def gaussian_weights(sigma, truncate=TRUNCATE):
    """The correlation weights ``scipy.ndimage.gaussian_filter1d(..., sigma)`` applies, bit for bit:
    radius ``r = int(truncate * sigma + 0.5)``, ``exp(-0.5 / sigma**2 * x**2)`` over
    ``x = -r .. r`` normalised by its sum.  Returns (weights, r)."""
    sigma = float(sigma)
    if not np.isfinite(sigma) or sigma <= 0:
        raise ValueError("sigma must be a positive number, got %r" % (sigma,))
    r = int(truncate * sigma + 0.5)
    if r > _lib.NOISE_MAX_RADIUS:
        raise ValueError("sigma %g gives a filter radius of %d cells; the device takes at most %d"
                         % (sigma, r, _lib.NOISE_MAX_RADIUS))
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return phi[::-1].copy(), r


def noiselevel_from_moments(moments, angles, first_nan_clear=False):
    """Mean and standard deviation of the high-passed directional curvature per orientation.

    ``moments``: the 20 numbers of ``sc_curvature_noise`` - (n, mean[3], C[6]) over all cells,
    then over the cells clear of the NaN boxes; C is the sum of centred products, upper triangle,
    row-major.  ``first_nan_clear``: the first orientation counts the second cell set (the grid
    held NaN cells).  ``sd = sqrt(max(var, 0))`` with the population variance (``nanstd``'s
    ddof 0); an empty cell set gives NaN.  Returns two lists of floats."""
    mo = np.asarray(moments, dtype=np.float64).reshape(2, 10)
    sets = []
    for n, mu, c in ((m[0], m[1:4], m[4:10]) for m in mo):
        cov = np.array([[c[0], c[1], c[2]],
                        [c[1], c[3], c[4]],
                        [c[2], c[4], c[5]]])
        sets.append((n, mu, cov))
    mean, sd = [], []
    for k, alpha in enumerate(np.asarray(angles, dtype=np.float64)):
        n, mu, cov = sets[1 if (k == 0 and first_nan_clear) else 0]
        if n == 0:
            mean.append(np.float64(np.nan))
            sd.append(np.float64(np.nan))
            continue
        ca, sa = np.cos(alpha), np.sin(alpha)
        v = np.array([ca ** 2, -2 * sa * ca, sa ** 2])
        var = (v @ cov @ v) / n
        mean.append(np.float64(v @ mu))
        sd.append(np.float64(np.sqrt(max(var, 0.0))))
    return mean, sd


def estimate_curvature_noiselevel(data, sigma=100., angles=None, device=0):
    """Noise level of the curvature of ``data`` as a function of direction
    (CalculationMixin._estimate_curvature_noiselevel, dem.py:152-179).

    ``data``: any grid-like object with ``_griddata`` / ``_georef_info`` (``dx``, ``dy``), like
    ``match`` takes - a ``scarplet_amd.DEMGrid`` or the reference's own.  ``sigma``: the low-pass
    filter's standard deviation in cells (the reference's 100); its radius ``int(4 sigma + 0.5)``
    may be at most ``_lib.NOISE_MAX_RADIUS`` (1 048 576) cells and may exceed the grid's sides.  The
    grid needs at least 3 x 3 cells, as every device path (``sc_set_dem``).  ``angles``:
    the orientations, by default ``np.linspace(0, np.pi, num=180)``.

    Returns ``(angles, mean, sd)``: an ndarray and two lists of floats, as the reference.  Like the
    reference, the grid keeps zeros where it held NaNs afterwards, and the first orientation counts
    only the cells farther than the filter radius from every NaN cell (NaN if there are none).
    Agrees with the reference to rounding (the reference's 180 filters are three here).

    The whole grid goes to the device: 8 + 24 bytes of device memory per cell (the grid and its
    three filtered planes), 3 more when it holds NaNs.  Work: 2 x 3 x (2 r + 8) float64 FMAs per cell."""
    from scarplet_amd.core import _context
    from scarplet_amd import WindowedTemplate as _WT
    weights, _ = gaussian_weights(sigma)
    if angles is None:
        angles = np.linspace(0, np.pi, num=180)
    angles = np.asarray(angles)
    z = data._griddata
    if not isinstance(z, np.ndarray) or z.dtype != np.float64 or not z.flags.c_contiguous:
        z = data._griddata = np.ascontiguousarray(z, dtype=np.float64)
    if z.ndim != 2 or min(z.shape) < 3:
        raise ValueError("data._griddata must be a 2-D array of at least 3 x 3 cells (the device's smallest "
                         "grid, sc_set_dem), got %s" % (z.shape,))
    nan_idx = np.isnan(z)
    has_nan = bool(nan_idx.any())
    z[nan_idx] = 0                                   # dem.py:84-86's write-through
    gi = data._georef_info
    dx = float(gi.dx)
    dy = float(gi.dy if gi.dy is not None else gi.dx)
    ny, nx = z.shape
    ctx = _context(device)
    ctx.set_dem(z, dx, dy, _WT.centred_axis(nx, dx), _WT.centred_axis(ny, dx))
    moments = ctx.curvature_noise(weights, nan_idx if has_nan else None)
    mean, sd = noiselevel_from_moments(moments, angles, first_nan_clear=has_nan)
    return angles, mean, sd
