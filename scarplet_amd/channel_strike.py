"""A channel's width and depth in windows along the strike of a reach, on the device (docs/channels.md, "Width along a
reach").

``fit_channel_segments`` gives a whole reach one width; ``fit_channels_along_strike`` gives the width and the depth as
functions of the position along the reach - downstream hydraulic geometry: at stations spaced ``step`` apart along every
reach's strike, the model of ``fit_channel_segments`` is fitted to the profiles of the cells within ``window / 2`` of the
station (sc_channel_strike, include/scarplet_hip.h).  The windows are cut here, in float64 numpy, by
``fit_along_strike``'s rules, and handed over as integer ranges.
"""
import collections

import numpy as np

from scarplet_amd import _lib, channel_segments, channels, profiles, strike

# the library's row under the channel's names (kt carries f), what follows from f and a, then the station's own
FIT_FIELDS = [(channels._RENAMED.get(f, f), _lib.STRIKE_FIT_DTYPE.fields[f][0]) for f in _lib.STRIKE_FIT_DTYPE.names] + \
    [(f, np.float64) for f in channels.DERIVED[:-2]] + \
    [("shift_mean", np.float64), ("t", np.float64), ("row", np.float64), ("col", np.float64)]
FIT_DTYPE = np.dtype(FIT_FIELDS)

# the first of what check_args returns, in the order Context.channel_strike takes it
Args = collections.namedtuple("Args", "cells sa ca seg_start seg_label seg_win_start win_lo win_hi frequencies h w D mode de "
                                      "delta min_samples min_profiles")


def check_args(shape, de, cells, labels, angle, half_length, frequencies, swath, window, step, max_shift, depth, delta,
               min_samples, min_profiles, with_t=False):
    """What the library takes, validated and normalised; ValueError otherwise.  The arguments shared with
    ``fit_channel_segments`` go through ``channel_segments.check_args``, the park's cap per reach included; ``window`` and
    ``step`` through ``strike.check_window``.  The cells are then sorted by (label, t, input position) and the windows cut
    along the axial mean of each reach's angles (``strike.cut``).  Returns the arguments of ``Context.channel_strike`` and
    (centre, row, col): each window's ``u_k`` and the means of its cells' rows and columns (NaN for an empty window); with
    ``with_t`` also the along-strike coordinate of every cell handed over (``channel_strike_bootstrap`` cuts its blocks on
    it)."""
    s = channel_segments.check_args(shape, de, cells, labels, angle, half_length, frequencies, swath, max_shift, depth, delta,
                                    min_samples, min_profiles)
    win, stp = strike.check_window(window, step, s.de)
    (idx, sa, ca, seg_win_start, win_lo, win_hi), where, t = strike.cut(shape, s.de, cells, angle, s, win, stp)
    args = Args(idx, sa, ca, s.seg_start, s.seg_label, seg_win_start, win_lo, win_hi, s.frequencies, s.h, s.w, s.D, s.mode,
                s.de, s.delta, s.min_samples, s.min_profiles)
    return (args, where, t) if with_t else (args, where)


def _run(ctx, args, where, nx, return_curve, z=None):
    """The call on ``args`` (check_args' record) and its result as ``fit_channels_along_strike`` returns it."""
    rows, curve, shift_sum = ctx.channel_strike(*args, curve=bool(return_curve), z=z)
    # (the formulas of fit_channels' table, on rows that carry no cell and no shift)
    full = np.zeros(len(rows), dtype=_lib.PROFILE_SHIFT_DTYPE)
    for f in ("status", "kt", "kt_lo", "kt_hi", "a"):
        full[f] = rows[f]
    derived = channels._table(full, nx, 0.0, 0.0)
    out = np.zeros(len(rows), dtype=FIT_DTYPE)
    for f in rows.dtype.names:
        out[channels._RENAMED.get(f, f)] = rows[f]
    for f in channels.DERIVED[:-2]:
        out[f] = derived[f]
    fitted = (rows["status"] & 1) == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        out["shift_mean"] = np.where(fitted, args.de * shift_sum / rows["n_profiles"], np.nan)
    out["t"], out["row"], out["col"] = where
    return (out, curve) if return_curve else out


def fit_channels_along_strike(data, cells, labels, angle, half_length, frequencies, swath=0, window=None, step=None,
                              max_shift=0, depth="profile", delta=1.0, min_samples=4, min_profiles=1, return_curve=False,
                              device=0):
    """The width and the depth of every reach as functions of the position along its strike (docs/channels.md, "Width along
    a reach").

    ``data``, ``cells``, ``labels``, ``angle``, ``half_length``, ``frequencies``, ``swath``, ``max_shift``, ``depth``,
    ``delta``, ``min_samples`` and ``min_profiles`` are those of ``sl.fit_channel_segments``; ``window`` and ``step`` those
    of ``sl.fit_along_strike``: along the strike of each reach (the axial mean of its cells' angles; a cell lies at ``t =
    de (row cos a_s + col sin a_s)``) stations are placed ``step`` apart, centred on the reach, and at each the model of
    ``fit_channel_segments`` is fitted to the profiles of the cells with ``|t - u_k| <= window / 2``.  ``window`` is
    required, in data units, at least the cell size; ``step`` defaults to ``window / 2`` and must lie between the cell size
    and the window.  Every profile keeps the shifts it takes on its own: they are not re-fitted per window.  A frequency
    that is dead in one usable profile of a window is dead for that window.  A window with fewer than ``min_profiles``
    usable profiles or less than one degree of freedom is not fitted (``status`` 1, indices -1, NaN floats); 33: every
    frequency is dead.  With ``depth="segment"`` the curve is ``SSpp - Q_i``, a subtraction (docs/strike.md, "The
    subtraction"); the index and ``a`` have none.

    Returns a structured array, one row per (label, station), sorted by both: ``label, station, n_cells, n_profiles, n, dof,
    f_index, lo_index, hi_index, status, f, f_lo, f_hi, a, sse, rmse``, then ``depth, sigma, width, width_lo, width_hi,
    area, curvature`` by the formulas of ``sl.fit_channels``, then ``shift_mean`` (the mean, in data units, of the usable
    profiles' centre shifts at the best frequency: how far the mapped trace lies off the fitted thalweg at the station; NaN
    where the window is not fitted), ``t`` (the station's along-strike coordinate ``u_k``) and ``row, col`` (the float64
    means of the rows and columns of the window's cells; NaN for an empty window).  ``return_curve`` adds the (NW, F) sse
    curves.  The same bytes on every run."""
    z, de = profiles._dem_of(data)
    args, where = check_args(z.shape, de, cells, labels, angle, half_length, frequencies, swath, window, step, max_shift, depth,
                             delta, min_samples, min_profiles)
    z = np.ascontiguousarray(z, dtype=np.float64)
    from scarplet_amd.core import _context
    return _run(_context(device), args, where, z.shape[1], return_curve, z=z)
