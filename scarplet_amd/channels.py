"""Channel depth and width across a trace, on the device (docs/channels.md).

A ``Channel`` search (the Ricker wavelet) returns planes and ``sl.extract_traces`` thins them into lines.
``fit_channels`` is to such a line what ``fit_profiles`` is to a scarp's: an elevation profile is cut across the trace at
each cell and the surface of which the Ricker wavelet is the curvature, a Gaussian trough
``z(s) = c0 + b s + a exp(-(pi f (s - d de))^2)``, is fitted to it for every frequency of a grid and every centre shift
``d``.  The best frequency, the depth ``-a``, the width and the interval of frequencies the profile does not tell apart
come back as one row per cell (sc_channel_profiles, include/scarplet_hip.h).
"""
import collections
import math

import numpy as np

from scarplet_amd import _lib, profiles

MAX_ARG = 6.0                                                          # SC_CHANNEL_MAX_ARG: pi f de at most

# the library's row under the channel's names: kt carries f
_RENAMED = {"kt_index": "f_index", "kt": "f", "kt_lo": "f_lo", "kt_hi": "f_hi"}
ROW_FIELDS = [(_RENAMED.get(f, f), _lib.PROFILE_SHIFT_DTYPE.fields[f][0]) for f in _lib.PROFILE_SHIFT_DTYPE.names]
DERIVED = ("depth", "sigma", "width", "width_lo", "width_hi", "area", "curvature", "centre_row", "centre_col")
FIT_FIELDS = [("row", np.int64), ("col", np.int64)] + ROW_FIELDS + [(f, np.float64) for f in DERIVED]
FIT_DTYPE = np.dtype(FIT_FIELDS)

# what check_args returns, in the order Context.channel_profiles takes it; then the angles, for the centres
Args = collections.namedtuple("Args", "cells sa ca frequencies h w D de delta min_samples")


def check_frequencies(frequencies, de):
    """The frequency grid as float64, 1-D and C-contiguous; ValueError otherwise."""
    try:
        f = np.atleast_1d(np.asarray(frequencies, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError("frequencies must be numbers")
    if f.ndim != 1 or f.size < 1:
        raise ValueError("frequencies must be a non-empty 1-D sequence")
    if f.size > _lib.CHANNEL_MAX_FREQS:
        raise ValueError("%d frequencies: more than %d" % (f.size, _lib.CHANNEL_MAX_FREQS))
    if not (np.all(np.isfinite(f)) and np.all(f > 0) and np.all(np.diff(f) > 0)):
        raise ValueError("frequencies must be finite, positive and strictly increasing")
    if not (np.pi * f[-1]) * de <= MAX_ARG:
        raise ValueError("frequency %r at a cell size of %r: pi f de is more than %r, a trough narrower than a cell shows"
                         % (float(f[-1]), de, MAX_ARG))
    return np.ascontiguousarray(f)


def check_args(shape, de, cells, angle, half_length, frequencies, swath, max_shift, delta, min_samples):
    """Args validated and normalised for the library; ValueError otherwise.  ``cells``, ``angle``, ``half_length``,
    ``swath``, ``delta`` and ``min_samples`` are ``fit_profiles``' (profiles.check_args); ``max_shift`` is in data units:
    D = floor(max_shift / de)."""
    a = profiles.check_args(shape, de, cells, angle, half_length, swath, [1.0], delta, min_samples)
    f = check_frequencies(frequencies, a.de)
    if max_shift is None:
        raise ValueError("max_shift must be a number (0: the centre stays at the cell)")
    D = profiles.check_shift(max_shift, False, a.de, a.h, a.min_samples)
    return Args(a.cells, a.sa, a.ca, f, a.h, a.w, D, a.de, a.delta, a.min_samples)


def _table(rows, nx, sa, ca, label=None):
    """The library's rows -> the Python table: row, col, the row's fields under the channel's names, what follows from f
    and a (NaN where the row is not fitted), ``label`` when given."""
    out = np.zeros(len(rows), dtype=np.dtype(FIT_FIELDS + ([] if label is None else [("label", np.int32)])))
    for f in rows.dtype.names:
        out[_RENAMED.get(f, f)] = rows[f]
    out["row"] = rows["cell"] // nx
    out["col"] = rows["cell"] % nx
    f, a = rows["kt"], rows["a"]
    fitted = (rows["status"] & 1) == 0
    nan = np.full(len(rows), np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        out["depth"] = -a
        out["sigma"] = 1.0 / (math.sqrt(2.0) * np.pi * f)
        out["width"] = 2.0 * math.sqrt(math.log(2.0)) / (np.pi * f)
        out["width_lo"] = 2.0 * math.sqrt(math.log(2.0)) / (np.pi * rows["kt_hi"])
        out["width_hi"] = 2.0 * math.sqrt(math.log(2.0)) / (np.pi * rows["kt_lo"])
        out["area"] = -a / (math.sqrt(np.pi) * f)
        out["curvature"] = -2.0 * (np.pi * f) ** 2 * a
    out["centre_row"] = np.where(fitted, out["row"] - rows["shift_index"] * sa, nan)
    out["centre_col"] = np.where(fitted, out["col"] + rows["shift_index"] * ca, nan)
    if label is not None:
        out["label"] = label
    return out


def _run(ctx, args, nx, return_curve, return_shift, z=None, label=None):
    """The call on ``args`` (check_args' record) and its result as ``fit_channels`` returns it."""
    rows, curve, plane = ctx.channel_profiles(*args, curve=bool(return_curve), shift_plane=bool(return_shift), z=z)
    res = [_table(rows, nx, args.sa, args.ca, label)] + ([curve] if return_curve else []) + ([plane] if return_shift else [])
    return res[0] if len(res) == 1 else tuple(res)


def fit_channels(data, cells, angle, half_length, frequencies, swath=0, max_shift=0, delta=1.0, min_samples=4,
                 return_curve=False, return_shift=False, device=0):
    """Fit a Gaussian trough to elevation profiles cut across the strike at ``cells`` (docs/channels.md).

    ``data``, ``cells``, ``angle``, ``half_length``, ``swath``, ``delta`` and ``min_samples`` as ``sl.fit_profiles`` takes
    them; the profile runs along (row, col) = (-sin a, cos a).  ``frequencies``: the grid of the Ricker frequency ``f`` -
    the ``age`` argument of ``sl.match(data, Channel, ...)`` -, finite, > 0, strictly increasing, at most 64, with
    ``pi f de <= 6``.  ``max_shift`` (data units) lets the trough's centre sit ``d`` cells along the profile,
    ``|d| <= D = floor(max_shift / de)``.  For every cell, every frequency and every shift the profile is fitted by
    ``c0 + b s + a exp(-(pi f (s - d de))^2)`` in float64; every frequency takes the shift of its smallest sum of squared
    residuals (tried in the order 0, -1, +1, ...), the frequency with the smallest of those wins, and ``lo_index ..
    hi_index`` is the run of frequencies around it whose sse stays within ``sse_min (1 + delta / dof)``,
    ``dof = n - 3 - (D > 0)``.

    Returns a structured array, one row per cell in input order: ``row, col, cell, n, f_index, lo_index, hi_index, status,
    f, f_lo, f_hi, a, b, c0, sse, rmse, shift_index, shift``, then ``depth`` (= -a: > 0 for a channel, < 0 for a ridge),
    ``sigma`` (= 1 / (sqrt(2) pi f)), ``width`` (= 2 sqrt(ln 2) / (pi f), the full width at half depth), ``width_lo`` and
    ``width_hi`` (from ``f_hi`` and ``f_lo``), ``area`` (= -a / (sqrt(pi) f), of the cross-section), ``curvature``
    (= -2 (pi f)^2 a, to be compared with the search's ``amp``), ``centre_row`` and ``centre_col`` (the cell moved by
    ``shift_index`` along the profile: the fitted thalweg).  ``status`` 1: not fitted (NaN fields); 2 / 4: the interval is
    open at the low / high end of the grid; 8: ``|shift_index| == D`` with ``D > 0``; 33: no frequency could be fitted.
    ``return_curve`` adds the (K, F) sse curves, ``return_shift`` the (K, F) int8 plane of every frequency's shift.  The
    same bytes on every run."""
    z, de = profiles._dem_of(data)
    args = check_args(z.shape, de, cells, angle, half_length, frequencies, swath, max_shift, delta, min_samples)
    z = np.ascontiguousarray(z, dtype=np.float64)
    from scarplet_amd.core import _context
    return _run(_context(device), args, z.shape[1], return_curve, return_shift, z=z)
