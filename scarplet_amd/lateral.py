"""Strike-slip offsets across a trace, on the device (docs/lateral.md).

Every other measurement of the pipeline is vertical: the offset ``2 a`` of an erf step across the strike.  On a
strike-slip fault the slip is lateral: a channel or a ridge that crosses the trace is displaced ALONG it.
``lateral_offsets`` is the standard measurement of that displacement: at each station two fault-parallel topographic
profiles are cut, one on either side of the trace, and the lag along the strike at which the two agree best - each side
keeping a mean and a slope of its own - is the offset (sc_lateral_offsets, include/scarplet_hip.h).
"""
import collections
import math

import numpy as np

from scarplet_amd import _lib, profiles

# the table as Python returns it: where the station lies, then the library's row
FIT_FIELDS = [("row", np.int64), ("col", np.int64)] + \
    [(f, _lib.LATERAL_FIT_DTYPE.fields[f][0]) for f in _lib.LATERAL_FIT_DTYPE.names]
FIT_DTYPE = np.dtype(FIT_FIELDS)

# what check_args returns, in the order Context.lateral_offsets takes it
Args = collections.namedtuple("Args", "cells sa ca h q0 q1 D de delta min_samples")


def check_args(shape, de, cells, angle, half_length, near, far, max_offset, delta, min_samples):
    """(cells, sa, ca, h, q0, q1, D, de, delta, min_samples) validated and normalised for the library; ValueError
    otherwise.  The lengths are in data units: h = floor(half_length / de), q0 = floor(near / de), q1 = floor(far / de),
    D = floor(max_offset / de)."""
    ny, nx = (int(v) for v in shape)
    if ny < 2 or nx < 2:
        raise ValueError("the grid must be at least 2 x 2, got %d x %d" % (ny, nx))
    de = profiles._number(de, "the cell size")
    if de <= 0:
        raise ValueError("the cell size must be > 0")
    idx = profiles._cells_of(cells, ny, nx)
    if len(idx) > profiles.MAX_CELLS:
        raise ValueError("%d cells: more than 2^31 - 1" % len(idx))
    a = profiles._angles_of(angle, idx, ny, nx)
    hl, nr, fr, mo = (profiles._number(v, n) for v, n in ((half_length, "half_length"), (near, "near"), (far, "far"),
                                                          (max_offset, "max_offset")))
    if hl < 0:
        raise ValueError("half_length must be >= 0")
    h = int(math.floor(hl / de))
    if h < 1:
        raise ValueError("half_length %r is %d cells of %r: at least 1 is needed" % (half_length, h, de))
    if h > _lib.PROFILE_MAX_HALF:
        raise ValueError("half_length %r is %d cells: more than %d" % (half_length, h, _lib.PROFILE_MAX_HALF))
    if nr < de:
        raise ValueError("near must be at least the cell size %r, got %r" % (de, near))
    if fr < nr:
        raise ValueError("far must be at least near (%r), got %r" % (near, far))
    q0, q1 = int(math.floor(nr / de)), int(math.floor(fr / de))
    if q1 > _lib.LATERAL_MAX_FAR:
        raise ValueError("far %r is %d cells: more than %d" % (far, q1, _lib.LATERAL_MAX_FAR))
    if q1 - q0 + 1 > _lib.LATERAL_MAX_BAND:
        raise ValueError("near %r to far %r are %d lines: more than %d" % (near, far, q1 - q0 + 1, _lib.LATERAL_MAX_BAND))
    if mo < 0:
        raise ValueError("max_offset must be >= 0, got %r" % (max_offset,))
    D = int(math.floor(mo / de))
    if D > _lib.LATERAL_MAX_LAG:
        raise ValueError("max_offset %r is %d cells: more than %d" % (max_offset, D, _lib.LATERAL_MAX_LAG))
    d = profiles._number(delta, "delta")
    if d < 0:
        raise ValueError("delta must be >= 0, got %r" % (delta,))
    ms = profiles._integer(min_samples, 3, 2 * h + 1, "min_samples must be an integer",
                           "min_samples must lie in 3..%d (the points of the window)" % (2 * h + 1))
    return Args(idx, np.sin(a), np.cos(a), h, q0, q1, D, de, d, ms)


def _table(rows, nx, label=None):
    """The library's rows -> the Python table (row, col, the row's fields; ``label`` when given)."""
    dt = np.dtype(FIT_FIELDS + ([] if label is None else [("label", np.int32)]))
    out = np.zeros(len(rows), dtype=dt)
    for f in rows.dtype.names:
        out[f] = rows[f]
    out["row"] = rows["cell"] // nx
    out["col"] = rows["cell"] % nx
    if label is not None:
        out["label"] = label
    return out


def lateral_offsets(data, cells, angle, half_length, near, far, max_offset, delta=1.0, min_samples=8, return_curve=False,
                    device=0):
    """The strike-slip offset across the trace at ``cells``, by cross-correlation of fault-parallel profiles
    (docs/lateral.md).

    ``data``, ``cells`` and ``angle`` are those of ``sl.fit_profiles``: the strike runs along (row, col) =
    (cos a, sin a), the ``+q`` side lies towards (-sin a, cos a).  All lengths are in data units.  On the ``-q`` side
    the profile ``u`` is cut along the strike over ``|t| <= half_length``, each point the mean of the lines ``near ..
    far`` away from the trace (one line per cell); on the ``+q`` side ``v`` likewise over ``|t| <= half_length +
    max_offset``.  For every lag ``d`` with ``|d| <= max_offset`` (whole cells) ``u_t`` and ``v_{t + d}`` are each
    reduced by a mean and a line of their own - a vertical step and a differential tilt across the fault cost nothing -
    and the mean squared difference of what is left is ``mse_d``.  The lag with the smallest mse wins (tried in the
    order 0, -1, +1, ...); ``lo .. hi`` is the run of lags around it whose mse stays within ``mse (1 + delta /
    (n - 2))``, and ``offset`` refines the lag by a parabola through its neighbours.  A lag with fewer than
    ``min_samples`` common points is skipped (``status`` gains 16); a station without a fitted lag has ``status`` 1, zero
    integers and NaN floats.  ``status`` 2 / 4 flag an interval that reaches the lower / upper end of the lags, 8 a best
    lag at either end.

    ``offset > 0``: the features of the ``+q`` side lie displaced along (cos a, sin a) relative to the ``-q`` side -
    right-lateral on a north-up raster, whichever of the strike's two angles was passed.

    Returns a structured array, one row per cell in input order (repeats allowed): ``row, col, cell, n, lag, lo, hi,
    status, offset, offset_lo, offset_hi, mse, rho, dz, tilt`` - ``rho`` the correlation of the two residuals at the
    best lag, ``dz`` and ``tilt`` the ``+q`` side's mean and slope less the ``-q`` side's - and the (K, 2 D + 1) mse
    curves (column ``d + D``) when ``return_curve``.  The same bytes on every run."""
    z, de = profiles._dem_of(data)
    args = check_args(z.shape, de, cells, angle, half_length, near, far, max_offset, delta, min_samples)
    z = np.ascontiguousarray(z, dtype=np.float64)
    from scarplet_amd.core import _context
    return _run(_context(device), args, z.shape[1], return_curve, z=z)


def _run(ctx, args, nx, return_curve, z=None, label=None):
    rows, curve = ctx.lateral_offsets(*args, curve=bool(return_curve), z=z)
    out = _table(rows, nx, label)
    return (out, curve) if return_curve else out
