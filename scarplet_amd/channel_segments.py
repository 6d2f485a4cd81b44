"""One channel width per reach, fitted jointly on the device (docs/channels.md, "One width per reach").

``fit_channels`` measures every cell of a trace on its own; a mapped reach gets ONE width with ONE interval.
``fit_channel_segments`` cuts the same profiles (the same samples, bit for bit), lets every profile choose its own centre
shift at every frequency as ``fit_channels`` chooses it, and pools the profiles of a reach per frequency: with
``depth="profile"`` every profile keeps a depth of its own, with ``depth="segment"`` the depth is the reach's, the
fixed-effects fit of ``fit_segments`` on the Gaussian column (sc_channel_segments, include/scarplet_hip.h).
"""
import collections

import numpy as np

from scarplet_amd import _lib, channels, profiles, segments

DEPTH_MODES = {"profile": _lib.CHANNEL_DEPTH_PROFILE, "segment": _lib.CHANNEL_DEPTH_SEGMENT}

# the library's row under the channel's names (kt carries f), then what follows from f and a
FIT_FIELDS = [(channels._RENAMED.get(f, f), _lib.SEGMENT_FIT_DTYPE.fields[f][0]) for f in _lib.SEGMENT_FIT_DTYPE.names] + \
    [(f, np.float64) for f in channels.DERIVED[:-2]]
FIT_DTYPE = np.dtype(FIT_FIELDS)
CELL_FIELDS = [("row", np.int64), ("col", np.int64)] + \
    [(f, _lib.CHANNEL_SEGMENT_CELL_DTYPE.fields[f][0]) for f in _lib.CHANNEL_SEGMENT_CELL_DTYPE.names] + \
    [("shift", np.float64), ("depth", np.float64), ("centre_row", np.float64), ("centre_col", np.float64), ("label", np.int32)]
CELL_DTYPE = np.dtype(CELL_FIELDS)

# what check_args returns: the arguments of Context.channel_segments in its order, then the sort's permutation of the kept
# cells and their input positions
Args = collections.namedtuple("Args", "cells sa ca seg_start seg_label frequencies h w D mode de delta min_samples "
                                      "min_profiles order kept")


def check_args(shape, de, cells, labels, angle, half_length, frequencies, swath, max_shift, depth, delta, min_samples,
               min_profiles):
    """What the library takes, validated and normalised; ValueError otherwise.  ``cells``, ``labels``, ``angle``,
    ``half_length``, ``swath``, ``delta``, ``min_samples`` and ``min_profiles`` go through ``segments.check_args`` (cells of
    label <= 0 dropped, the rest grouped by label with a stable sort); ``frequencies`` and ``max_shift`` are
    ``fit_channels``' (``channels.check_frequencies``; D = floor(max_shift / de)).  The park -
    ``_lib.channel_segment_park(h, F)`` bytes per cell, a reach at a time - must hold every reach."""
    if depth not in DEPTH_MODES:
        raise ValueError("depth must be 'profile' or 'segment', got %r" % (depth,))
    a = segments.check_args(shape, de, cells, labels, angle, half_length, swath, [1.0], delta, min_samples, min_profiles)
    f = channels.check_frequencies(frequencies, a.de)
    if max_shift is None:
        raise ValueError("max_shift must be a number (0: the centre stays at the cell)")
    D = profiles.check_shift(max_shift, False, a.de, a.h, a.min_samples)
    segments._check_cap(a.seg_start, _lib.channel_segment_cap(a.h, len(f)), " and number of frequencies")
    return Args(a.cells, a.sa, a.ca, a.seg_start, a.seg_label, f, a.h, a.w, D, DEPTH_MODES[depth], a.de, a.delta,
                a.min_samples, a.min_profiles, a.order, a.kept)


def _run(ctx, args, nx, return_cells, return_curve, return_shift, z=None):
    """The call on ``args`` (check_args' record) and its result as ``fit_channel_segments`` returns it: the table, then what
    was asked for of the cell table, the curves and the shifts - per cell in input order."""
    call, order = args[:-2], args.order
    rows, tab, curve, plane = ctx.channel_segments(*call, cell_table=bool(return_cells), curve=bool(return_curve),
                                                   shift_plane=bool(return_shift), z=z)
    # (the formulas of fit_channels' table, on rows that carry no cell and no shift)
    full = np.zeros(len(rows), dtype=_lib.PROFILE_SHIFT_DTYPE)
    for f in ("status", "kt", "kt_lo", "kt_hi", "a"):
        full[f] = rows[f]
    derived = channels._table(full, nx, 0.0, 0.0)
    table = np.zeros(len(rows), dtype=FIT_DTYPE)
    for f in rows.dtype.names:
        table[channels._RENAMED.get(f, f)] = rows[f]
    for f in channels.DERIVED[:-2]:
        table[f] = derived[f]
    res = [table]
    if return_cells or return_shift:
        back = np.empty(len(order), dtype=np.int64)                    # sorted position of each kept cell
        back[order] = np.arange(len(order))
    if return_cells:
        ct = np.zeros(len(tab), dtype=CELL_DTYPE)
        for f in tab.dtype.names:
            ct[f] = tab[f][back]
        ct["row"] = ct["cell"] // nx
        ct["col"] = ct["cell"] % nx
        ct["label"] = np.repeat(args.seg_label, np.diff(args.seg_start))[back]
        unfit = np.isnan(ct["b"])
        ct["shift"] = np.where(unfit, np.nan, ct["shift_index"] * args.de)
        ct["depth"] = -ct["a"]
        ct["centre_row"] = np.where(unfit, np.nan, ct["row"] - ct["shift_index"] * args.sa[back])
        ct["centre_col"] = np.where(unfit, np.nan, ct["col"] + ct["shift_index"] * args.ca[back])
        res.append(ct)
    if return_curve:
        res.append(curve)
    if return_shift:
        res.append(np.ascontiguousarray(plane[back]))
    return res[0] if len(res) == 1 else tuple(res)


def fit_channel_segments(data, cells, labels, angle, half_length, frequencies, swath=0, max_shift=0, depth="profile",
                         delta=1.0, min_samples=4, min_profiles=1, return_cells=False, return_curve=False,
                         return_shift=False, device=0):
    """Fit ONE Gaussian trough width per reach to the profiles cut across the strike at its cells (docs/channels.md, "One
    width per reach").

    ``data``, ``cells``, ``labels``, ``angle``, ``half_length``, ``swath``, ``delta``, ``min_samples`` and ``min_profiles``
    are those of ``sl.fit_segments``: the cells of one label are one reach, cells of label <= 0 are dropped.
    ``frequencies`` and ``max_shift`` are those of ``sl.fit_channels``.  Every usable profile (at least ``min_samples``
    valid points on either side) takes, at every frequency, the centre shift ``fit_channels`` would give it.  With
    ``depth="profile"`` the frequency is the reach's and depth, intercept, slope and centre are each profile's own: the
    pooled sse is the sum of the profiles' own, ``a`` is the mean of their depths' ``a`` at the best frequency and ``dof = n
    - (3 + (D > 0)) n_profiles``.  With ``depth="segment"`` the amplitude is the reach's too, the joint fit of
    ``sl.fit_segments(..., max_shift=...)`` on the Gaussian column, ``dof = n - 2 n_profiles - 1 - (D > 0) n_profiles``.
    The frequency with the smallest pooled sse wins; ``lo_index .. hi_index`` is the run of frequencies around it whose sse
    stays within ``sse_min (1 + delta / dof)``.  A frequency that is dead in one usable profile is dead for the reach.

    Returns a structured array, one row per distinct label in ascending order: ``label, n_cells, n_profiles, n, dof,
    f_index, lo_index, hi_index, status, f, f_lo, f_hi, a, sse, rmse``, then ``depth, sigma, width, width_lo, width_hi, area,
    curvature`` by the formulas of ``sl.fit_channels``.  ``status`` 1: not fitted (fewer than ``min_profiles`` usable
    profiles or ``dof < 1``; NaN fields); 2 / 4: the interval is open at the low / high end; 8: a usable profile's shift at
    the best frequency is the end of its range; 33: every frequency is dead.  ``return_cells`` adds the per-cell table in
    input order (``row, col, cell, used, n, a, b, c0, sse, shift_index, shift, depth, centre_row, centre_col, label`` at the
    reach's best frequency; ``a`` the profile's own with ``depth="profile"``, the reach's with ``depth="segment"``),
    ``return_curve`` the (S, F) pooled curves and ``return_shift`` the (K_kept, F) int8 plane of every profile's shift at
    every frequency, in that order.  The same bytes on every run."""
    z, de = profiles._dem_of(data)
    args = check_args(z.shape, de, cells, labels, angle, half_length, frequencies, swath, max_shift, depth, delta,
                      min_samples, min_profiles)
    z = np.ascontiguousarray(z, dtype=np.float64)
    from scarplet_amd.core import _context
    return _run(_context(device), args, z.shape[1], return_cells, return_curve, return_shift, z=z)
