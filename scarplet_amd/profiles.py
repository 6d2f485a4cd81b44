"""Scarp-profile dating across a trace, on the device (docs/profiles.md).

``sl.match`` finds per cell the curvature template that fits best, ``sl.extract_traces`` turns that into lines.
``fit_profiles`` is the classical check of morphologic dating on such a line: an elevation profile is cut across
the trace at each cell, the diffusion scarp ``z(s) = c0 + b s + a erf(s / (2 sqrt(kt)))`` is fitted to it for every
age of a grid, and the best age, the offset ``2 a``, the far-field slope ``b`` and the interval of ages the profile
does not tell apart come back as one row per cell (sc_fit_profiles, include/scarplet_hip.h) - instead of a Python
loop of ``map_coordinates`` and ``lstsq`` over the cells.
"""
import collections
import math
import operator

import numpy as np

from scarplet_amd import _lib, _plan

MAX_CELLS = 2 ** 31 - 1

# the table as Python returns it: where the cell lies, the library's row, the scarp's offset
FIT_FIELDS = [("row", np.int64), ("col", np.int64)] + \
    [(f, _lib.PROFILE_DTYPE.fields[f][0]) for f in _lib.PROFILE_DTYPE.names] + [("height", np.float64)]
FIT_DTYPE = np.dtype(FIT_FIELDS)
# ... and with max_shift: the best age's shift, in cells and in data units
SHIFT_FIT_FIELDS = FIT_FIELDS + [("shift_index", np.int32), ("shift", np.float64)]
SHIFT_FIT_DTYPE = np.dtype(SHIFT_FIT_FIELDS)
# ... and with weights or a robust loss: the loss and the scale of the best age, the points it down-weighted, and the best
# age of the plain weighted fit
ROBUST_FIT_FIELDS = FIT_FIELDS + [("loss", np.float64), ("scale", np.float64), ("n_down", np.int32), ("ls_index", np.int32)]
ROBUST_FIT_DTYPE = np.dtype(ROBUST_FIT_FIELDS)
# ... and with max_width: the half-width of the best age's initial ramp, in cells and in data units, and its gradient
RAMP_FIT_FIELDS = FIT_FIELDS + [("width_index", np.int32), ("width", np.float64), ("initial_slope", np.float64)]
RAMP_FIT_DTYPE = np.dtype(RAMP_FIT_FIELDS)
# ... and with refine: the minimum and the interval off the grid, after ``height``
FINE_FIT_FIELDS = FIT_FIELDS + [(f, np.float64) for f in _lib.FINE_FLOATS] + [("status_fine", np.int32)]
FINE_FIT_DTYPE = np.dtype(FINE_FIT_FIELDS)
ROBUST_LOSSES = {"huber": (_lib.ROBUST_HUBER, 1.345), "tukey": (_lib.ROBUST_TUKEY, 4.685)}

# what check_args returns, in the order Context.fit_profiles takes it
Args = collections.namedtuple("Args", "cells sa ca ages h w de delta min_samples")
# what check_options returns: D or None, check_robust's tuple or None, check_width's tuple or None, R or None - the
# keywords of _run
Options = collections.namedtuple("Options", "shift robust ramp refine")


def _number(x, name):
    if isinstance(x, (bool, np.bool_)):
        raise ValueError("%s must be a number" % name)
    try:
        v = float(x)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number" % name)
    if not math.isfinite(v):
        raise ValueError("%s must be finite, got %r" % (name, x))
    return v


def _integer(x, lo, hi, not_int, out_of_range):
    """``x`` as an int in lo..hi (``hi`` None: no upper end); ValueError in the caller's words otherwise: ``not_int`` for a
    bool and, with the value, for whatever else is no integer; ``out_of_range``, with the value."""
    if isinstance(x, (bool, np.bool_)):
        raise ValueError(not_int)
    try:
        v = operator.index(x)
    except TypeError:
        raise ValueError("%s, got %r" % (not_int, x))
    if v < lo or (hi is not None and v > hi):
        raise ValueError("%s, got %r" % (out_of_range, x))
    return v


def _cells_of(cells, ny, nx):
    """Linear indices (int64, 1-D) of ``cells``: linear indices, a (rows, cols) pair, or a bool plane."""
    if isinstance(cells, tuple):
        if len(cells) != 2:
            raise ValueError("cells as a tuple must be (rows, cols)")
        r, c = (np.asarray(v) for v in cells)
        if r.shape != c.shape or r.ndim > 1:
            raise ValueError("rows and cols of cells must be 1-D and of one length")
        r, c = np.atleast_1d(r), np.atleast_1d(c)
        for v in (r, c):
            if v.size and v.dtype.kind not in "iu":
                raise ValueError("rows and cols of cells must be integers")
        if r.size and (r.min() < 0 or r.max() >= ny or c.min() < 0 or c.max() >= nx):
            raise ValueError("cells outside the %d x %d grid" % (ny, nx))
        return r.astype(np.int64) * nx + c.astype(np.int64)
    arr = np.asarray(cells)
    if arr.dtype == np.bool_:
        if arr.shape != (ny, nx):
            raise ValueError("a bool plane of cells must have the grid's shape %r, got %r" % ((ny, nx), arr.shape))
        return np.flatnonzero(arr.ravel()).astype(np.int64)
    if arr.ndim > 1:
        raise ValueError("cells must be 1-D linear indices, a (rows, cols) tuple or a bool plane")
    arr = np.atleast_1d(arr)
    if arr.size == 0:
        return np.zeros(0, dtype=np.int64)
    if arr.dtype.kind not in "iu":
        raise ValueError("cells must be integers, got %s" % arr.dtype)
    if arr.min() < 0 or arr.max() >= ny * nx:
        raise ValueError("cells outside the %d x %d grid" % (ny, nx))
    return np.ascontiguousarray(arr, dtype=np.int64)


def _angles_of(angle, idx, ny, nx):
    """One orientation per cell (float64): a scalar, one per cell, or an (ny, nx) plane read at the cells."""
    try:
        a = np.asarray(angle, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("angle must be a number, one number per cell or an (ny, nx) plane")
    if a.ndim == 0:
        a = np.full(len(idx), float(a))
    elif a.ndim == 2:
        if a.shape != (ny, nx):
            raise ValueError("an angle plane must have the grid's shape %r, got %r" % ((ny, nx), a.shape))
        a = a.ravel()[idx]
    elif a.ndim != 1 or len(a) != len(idx):
        raise ValueError("angle must be a number, one number per cell (%d) or an (ny, nx) plane" % len(idx))
    if not np.all(np.isfinite(a)):
        raise ValueError("angle must be finite at every cell")
    return np.ascontiguousarray(a, dtype=np.float64)


def check_args(shape, de, cells, angle, half_length, swath, ages, delta, min_samples):
    """(cells, sa, ca, ages, h, w, delta, min_samples) validated and normalised for the library; ValueError
    otherwise.  ``half_length`` and ``swath`` are in data units: h = floor(half_length / de), w = floor(swath / de)."""
    ny, nx = (int(v) for v in shape)
    if ny < 2 or nx < 2:
        raise ValueError("the grid must be at least 2 x 2, got %d x %d" % (ny, nx))
    de = _number(de, "the cell size")
    if de <= 0:
        raise ValueError("the cell size must be > 0")
    idx = _cells_of(cells, ny, nx)
    if len(idx) > MAX_CELLS:
        raise ValueError("%d cells: more than 2^31 - 1" % len(idx))
    a = _angles_of(angle, idx, ny, nx)
    hl, sw = _number(half_length, "half_length"), _number(swath, "swath")
    if hl < 0 or sw < 0:
        raise ValueError("half_length and swath must be >= 0")
    h, w = int(math.floor(hl / de)), int(math.floor(sw / de))
    if h < 2:
        raise ValueError("half_length %r is %d cells of %r: at least 2 are needed" % (half_length, h, de))
    if h > _lib.PROFILE_MAX_HALF:
        raise ValueError("half_length %r is %d cells: more than %d" % (half_length, h, _lib.PROFILE_MAX_HALF))
    if w > _lib.PROFILE_MAX_SWATH:
        raise ValueError("swath %r is %d cells: more than %d" % (swath, w, _lib.PROFILE_MAX_SWATH))
    if ages is None:
        ages = _plan.age_grid()
    try:
        kt = np.atleast_1d(np.asarray(ages, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError("ages must be numbers")
    if kt.ndim != 1 or kt.size < 1:
        raise ValueError("ages must be a non-empty 1-D sequence")
    if kt.size > _lib.PROFILE_MAX_AGES:
        raise ValueError("%d ages: more than %d" % (kt.size, _lib.PROFILE_MAX_AGES))
    if not (np.all(np.isfinite(kt)) and np.all(kt > 0) and np.all(np.diff(kt) > 0)):
        raise ValueError("ages must be finite, positive and strictly increasing")
    d = _number(delta, "delta")
    if d < 0:
        raise ValueError("delta must be >= 0, got %r" % (delta,))
    ms = _integer(min_samples, 2, h, "min_samples must be an integer",
                  "min_samples must lie in 2..%d (the half-length in cells)" % h)
    return Args(idx, np.sin(a), np.cos(a), np.ascontiguousarray(kt), h, w, de, d, ms)


def check_shift(max_shift, return_shift, de, h, min_samples):
    """D = floor(max_shift / de), the range of the centre shift in cells, or None for ``max_shift=None``; ValueError
    otherwise.  ``de``, ``h`` and ``min_samples`` as check_args returns them."""
    if max_shift is None:
        if return_shift:
            raise ValueError("return_shift needs max_shift")
        return None
    ms = _number(max_shift, "max_shift")
    if ms < 0:
        raise ValueError("max_shift must be >= 0, got %r" % (max_shift,))
    D = int(math.floor(ms / de))
    top = min(_lib.PROFILE_MAX_SHIFT, h - min_samples)
    if D > top:
        raise ValueError("max_shift %r is %d cells: more than %d (at most %d, and half_length less min_samples)"
                         % (max_shift, D, top, _lib.PROFILE_MAX_SHIFT))
    return D


def check_robust(shape, weights, robust, tuning, iterations, robust_scale, max_shift):
    """None where neither ``weights`` nor ``robust`` is given, else (plane or None, loss, k, T, sigma or 0.0) for the
    library; ValueError otherwise.  A NaN in the plane marks ground without a weight, as a NaN of the DEM does."""
    if weights is None and robust is None:
        if tuning is not None or robust_scale is not None:
            raise ValueError("tuning and robust_scale need robust")
        return None
    if max_shift is not None:
        raise ValueError("weights and robust are not built together with max_shift")
    plane = None
    if weights is not None:
        try:
            plane = np.asarray(weights, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("weights must be a plane of numbers")
        if plane.shape != tuple(int(v) for v in shape):
            raise ValueError("weights must have the grid's shape %r, got %r" % (tuple(shape), plane.shape))
        if np.isinf(plane).any() or (plane < 0).any():
            raise ValueError("weights must be finite and >= 0")
        plane = np.ascontiguousarray(plane)
    if robust is None:
        if tuning is not None or robust_scale is not None:
            raise ValueError("tuning and robust_scale need robust")
        return plane, _lib.ROBUST_NONE, 0.0, 1, 0.0
    if not isinstance(robust, str) or robust not in ROBUST_LOSSES:
        raise ValueError("robust must be None, 'huber' or 'tukey', got %r" % (robust,))
    loss, k = ROBUST_LOSSES[robust]
    if tuning is not None:
        k = _number(tuning, "tuning")
        if k <= 0:
            raise ValueError("tuning must be > 0, got %r" % (tuning,))
    T = _integer(iterations, 1, _lib.ROBUST_MAX_ITER, "iterations must be an integer",
                 "iterations must lie in 1..%d" % _lib.ROBUST_MAX_ITER)
    sigma = 0.0
    if robust_scale is not None:
        sigma = _number(robust_scale, "robust_scale")
        if sigma <= 0:
            raise ValueError("robust_scale must be > 0, got %r" % (robust_scale,))
    return plane, loss, k, T, sigma


def check_width(max_width, initial_slope, return_width, de, h, min_samples, max_shift=None, weights=None, robust=None):
    """None for ``max_width=None``, else (M, mode, slope) for the library: M = floor(max_width / de), the range of the
    initial ramp's half-width in cells; ValueError otherwise.  ``de``, ``h`` and ``min_samples`` as check_args returns
    them."""
    if max_width is None:
        if initial_slope is not None:
            raise ValueError("initial_slope needs max_width")
        if return_width:
            raise ValueError("return_width needs max_width")
        return None
    if max_shift is not None or weights is not None or robust is not None:
        raise ValueError("max_width is not built together with max_shift, weights or robust")
    mw = _number(max_width, "max_width")
    if mw < 0:
        raise ValueError("max_width must be >= 0, got %r" % (max_width,))
    M = int(math.floor(mw / de))
    top = min(_lib.PROFILE_MAX_WIDTH, h - min_samples)
    if M > top:
        raise ValueError("max_width %r is %d cells: more than %d (at most %d, and half_length less min_samples)"
                         % (max_width, M, top, _lib.PROFILE_MAX_WIDTH))
    if initial_slope is None:
        return M, _lib.RAMP_FREE, 0.0
    g = _number(initial_slope, "initial_slope")
    if g <= 0:
        raise ValueError("initial_slope is a magnitude and must be > 0, got %r" % (initial_slope,))
    if M < 1:
        raise ValueError("initial_slope needs a max_width of at least one cell, got %r at a cell size of %r" % (max_width, de))
    return M, _lib.RAMP_SLOPE, g


def check_refine(refine, max_shift=None, weights=None, robust=None, max_width=None):
    """None for ``refine=None``, else R, the levels of 64 candidate ages below the grid (0, 1 or 2); ValueError otherwise."""
    if refine is None:
        return None
    if isinstance(refine, (bool, np.bool_)):
        raise ValueError("refine must be None, 0, 1 or 2, got %r" % (refine,))
    try:
        R = operator.index(refine)
    except TypeError:
        v = float(refine) if isinstance(refine, (float, np.floating)) else math.nan
        if not (math.isfinite(v) and v == math.floor(v)):
            raise ValueError("refine must be None, 0, 1 or 2, got %r" % (refine,))
        R = int(v)
    if R < 0 or R > _lib.PROFILE_MAX_REFINE:
        raise ValueError("refine must be None, 0, 1 or 2, got %r" % (refine,))
    if max_shift is not None or weights is not None or robust is not None or max_width is not None:
        raise ValueError("refine is not built together with max_shift, weights, robust or max_width")
    return R


def check_options(shape, args, max_shift, return_shift, weights, robust, tuning, iterations, robust_scale, max_width,
                  initial_slope, return_width, refine):
    """The options of ``fit_profiles`` beside ``args`` (check_args' record), checked in the one order that decides which
    ValueError a doubly wrong call gets: Options(shift, robust, ramp, refine) of check_shift, check_robust, check_width and
    check_refine."""
    D = check_shift(max_shift, return_shift, args.de, args.h, args.min_samples)
    rb = check_robust(shape, weights, robust, tuning, iterations, robust_scale, max_shift)
    rp = check_width(max_width, initial_slope, return_width, args.de, args.h, args.min_samples, max_shift, weights, robust)
    return Options(D, rb, rp, check_refine(refine, max_shift, weights, robust, max_width))


def _table(rows, nx, label=None):
    """The library's rows -> the Python table (row, col, the row's fields, height = 2 a; ``label`` when given)."""
    names = rows.dtype.names
    fields = SHIFT_FIT_FIELDS if "shift" in names else ROBUST_FIT_FIELDS if "loss" in names else \
        RAMP_FIT_FIELDS if "width" in names else FINE_FIT_FIELDS if "kt_fine" in names else FIT_FIELDS
    dt = np.dtype(fields + ([] if label is None else [("label", np.int32)]))
    out = np.zeros(len(rows), dtype=dt)
    for f in rows.dtype.names:
        out[f] = rows[f]
    out["row"] = rows["cell"] // nx
    out["col"] = rows["cell"] % nx
    out["height"] = 2.0 * rows["a"]
    if label is not None:
        out["label"] = label
    return out


def _dem_of(data):
    """(z, de) of a DEMGrid or of anything with its two attributes - shapes checked before anything is copied."""
    try:
        z = np.asarray(data._griddata)
        gi = data._georef_info
        de = float(gi.dx)
    except AttributeError:
        raise ValueError("data must be a DEMGrid")
    if z.ndim != 2:
        raise ValueError("data._griddata must be a 2-D array")
    return z, de


def fit_profiles(data, cells, angle, half_length, swath=0, ages=None, delta=1.0, min_samples=4, return_curve=False,
                 device=0, max_shift=None, return_shift=False, weights=None, robust=None, tuning=None, iterations=8,
                 robust_scale=None, max_width=None, initial_slope=None, return_width=False, refine=None):
    """Fit the diffusion scarp to elevation profiles cut across the strike at ``cells`` (docs/profiles.md).

    ``data``: the DEMGrid.  ``cells``: linear indices ``r * nx + c``, a ``(rows, cols)`` tuple, or a bool plane (its
    true cells in row-major order).  ``angle``: the orientation as ``sl.match`` returns it - a scalar, one per cell,
    or an (ny, nx) plane read at the cells; the profile runs along (row, col) = (-sin a, cos a).  ``half_length``
    and ``swath`` (half-width of the band averaged along the strike) are in data units.  ``ages``: the kt grid,
    strictly increasing (default: the search's, 10**0 .. 10**3.4).  For every cell and every age the profile is
    fitted by ``c0 + b s + a erf(s / (2 sqrt(kt)))`` in float64; the age with the smallest sum of squared residuals
    wins, and ``lo_index .. hi_index`` is the run of ages around it whose sse stays within
    ``sse_min (1 + delta / (n - 3))``.  A cell with fewer than ``min_samples`` valid points on either side has
    ``status`` 1 and NaN fields; ``status`` 2 / 4 flag an interval open at the young / old end of the grid.

    Returns a structured array, one row per cell in input order: ``row, col, cell, n, kt_index, lo_index, hi_index,
    status, kt, kt_lo, kt_hi, a, b, c0, sse, rmse, height`` (= 2 a) - and the (K, A) sse curves when
    ``return_curve``.  The same bytes on every run.

    ``max_shift`` (data units; None: the step stays at the cell) lets the step sit ``d`` cells along the profile,
    ``|d| <= floor(max_shift / de)``: ``a erf((s - d de) / (2 sqrt(kt)))``, the best ``d`` chosen for every age (tried
    in the order 0, -1, +1, ...).  The table gains ``shift_index`` (d of the best age) and ``shift`` (d de), the
    curves are the minima over d, one degree of freedom goes to the shift (``n - 4`` for ``n - 3`` when the range is
    not 0), and ``status`` gains 8 where ``|shift_index|`` is the end of the range.  ``return_shift`` adds the
    (K, A) int8 plane of every age's d, after the curves.

    ``weights`` (an (ny, nx) plane, finite and >= 0; NaN: ground without a weight) is sampled as the DEM is and weights
    every point of every sum; ``robust`` ("huber" or "tukey") adds ``iterations`` rounds of iteratively reweighted least
    squares per age with the constant ``tuning`` (default 1.345 / 4.685) on one scale per profile - ``robust_scale``, or
    1.4826 times the median absolute residual of the plain weighted fit's best age (docs/profiles.md, "Weights and
    robust fits").  The choice and the interval then run on the robust loss; the table gains ``loss``, ``scale``,
    ``n_down`` (the points the best age down-weighted) and ``ls_index`` (the best age before the robust step), ``sse``
    is the weighted sum of squared residuals of the final fit, ``rmse = sqrt(loss / (n - 3))``, the curves are the
    losses, and ``status`` gains 16 where the scale is 0 (the row is the weighted least squares row) and is 33 where no
    age kept enough points.  Neither is built together with ``max_shift``.

    ``max_width`` (data units; None: the scarp starts as a vertical step) fits the scarp that started as a ramp of
    half-width ``L = m de``, ``m <= floor(max_width / de)`` cells (docs/profiles.md, "The initial slope"): ``a g(s; kt, L)``
    with ``g = (F(s + L) - F(s - L)) / (2 L)``, ``F(x) = x erf(x / (2 sqrt(kt))) + 2 sqrt(kt / pi) exp(-x^2 / (4 kt))``,
    for ``a erf(...)``.  With ``initial_slope=None`` the width is free: every age takes the ``m`` of its smallest sse, and one
    degree of freedom goes to the width.  With ``initial_slope`` (a gradient magnitude, > 0: the angle of repose) every age
    takes the ``m >= 1`` whose ``|b + a / (m de)|`` is nearest to it, at ``n - 3`` degrees of freedom.  The table gains
    ``width_index`` (m of the best age), ``width`` (m de) and ``initial_slope`` (the signed ``b + a / (m de)``; +-inf at
    ``m = 0``), the curves are the chosen pairs' sse, and ``status`` gains 8 where ``width_index`` is the end of the range.
    ``return_width`` adds the (K, A) int8 plane of every age's m, after the curves.  Not built together with
    ``max_shift``, ``weights`` or ``robust``.

    ``refine`` (None: the answer is an age of the grid; 0, 1 or 2) adds that many levels of 64 candidate ages of the cell's
    own bracket below the grid - for the minimum and for either end of the interval (docs/profiles.md, "Continuous ages").
    Every field of the plain table keeps the plain call's bytes; the table gains ``kt_fine, kt_lo_fine, kt_hi_fine, a_fine,
    b_fine, c0_fine, sse_fine`` (<= ``sse``), ``rmse_fine, height_fine, status_fine``, and the curves stay the grid's.  Not
    built together with ``max_shift``, ``weights``, ``robust`` or ``max_width``."""
    z, de = _dem_of(data)
    args = check_args(z.shape, de, cells, angle, half_length, swath, ages, delta, min_samples)
    opts = check_options(z.shape, args, max_shift, return_shift, weights, robust, tuning, iterations, robust_scale, max_width,
                         initial_slope, return_width, refine)
    z = np.ascontiguousarray(z, dtype=np.float64)
    from scarplet_amd.core import _context
    return _run(_context(device), args, z.shape[1], return_curve, z=z, return_shift=return_shift, return_width=return_width,
                **opts._asdict())


def _run(ctx, args, nx, return_curve, z=None, label=None, shift=None, return_shift=False, robust=None, ramp=None,
         return_width=False, refine=None):
    """The call the options name, on ``args`` (check_args' record), and its result as ``fit_profiles`` returns it: the table,
    the curves when asked for, the int8 plane of the shifts or of the widths when asked for."""
    plane, want_plane, out = None, False, bool(return_curve)
    if refine is not None:
        rows, curve = ctx.fit_profiles_refine(*args, refine, curve=out, z=z)
    elif ramp is not None:
        M, mode, slope = ramp
        want_plane = bool(return_width)
        rows, curve, plane = ctx.fit_profiles_ramp(*args, M, mode=mode, slope=slope, curve=out, width_plane=want_plane, z=z)
    elif robust is not None:
        weights, loss, k, T, sigma = robust
        rows, curve = ctx.fit_profiles_robust(*args, weights=weights, loss=loss, tuning=k, iterations=T, scale=sigma, curve=out,
                                              z=z)
    elif shift is None:
        rows, curve = ctx.fit_profiles(*args, curve=out, z=z)
    else:
        want_plane = bool(return_shift)
        rows, curve, plane = ctx.fit_profiles(*args, curve=out, z=z, shift=shift, shift_plane=want_plane)
    res = [_table(rows, nx, label)] + ([curve] if return_curve else []) + ([plane] if want_plane else [])
    return res[0] if len(res) == 1 else tuple(res)
