"""Block-bootstrap intervals of a channel's width, depth and area at every station along a reach, on the device
(docs/channels.md, "Intervals per station").

``fit_channels_along_strike`` gives the width and the depth as functions of the position along a reach, each with the pooled
criterion's interval - too narrow, because neighbouring profiles are not independent (docs/channels.md, "Intervals per
reach").  ``bootstrap_channel_segments`` has the usable interval, but for a whole reach.
``bootstrap_channels_along_strike`` is the two together: in every window of ``fit_channels_along_strike`` the blocks of
neighbouring profiles along the strike are resampled with replacement and the window's frequency is chosen again in every
replicate (sc_channel_strike_bootstrap, include/scarplet_hip.h).  The windows and the blocks are cut here, in float64
numpy, and handed over as integers.
"""
import collections

import numpy as np

from scarplet_amd import _lib, bootstrap, channel_bootstrap, channel_strike, channels, strike_bootstrap

draw = strike_bootstrap.draw       # the block of a draw: the generator of bootstrap_along_strike, keyed by seed, label and station

BOOT_FIELDS = [(f, _lib.CHANNEL_STRIKE_BOOT_DTYPE.fields[f][0]) for f in _lib.CHANNEL_STRIKE_BOOT_DTYPE.names] + \
    channel_bootstrap.BOOT_FIELDS[len(_lib.CHANNEL_BOOT_DTYPE.names):] + [(f, np.float64) for f in ("t", "row", "col")]
BOOT_DTYPE = np.dtype(BOOT_FIELDS)

# the first of what check_args returns, in the order Context.channel_strike_bootstrap takes it
Args = collections.namedtuple("Args", "cells sa ca seg_start seg_label seg_win_start win_lo win_hi win_blk_start blk_hi "
                                      "frequencies h w D mode de min_samples min_profiles min_blocks R level seed")


def check_args(shape, de, cells, labels, angle, half_length, frequencies, swath, window, step, block_length, max_shift, depth,
               replicates, level, seed, min_samples, min_profiles, min_blocks):
    """What the library takes, validated and normalised; ValueError otherwise.  Everything shared with
    ``fit_channels_along_strike`` goes through ``channel_strike.check_args`` (``channel_segments.check_args``, the rules of
    the window and the step, ``strike.cut``), the resampling through ``bootstrap.check_resampling``.  The blocks of every
    window are then cut on the cells' along-strike coordinates (``strike_bootstrap.blocks_of``); a window whose block terms
    do not fit 64 KiB - ``nb F 16 > 65536`` - is refused.  Returns the arguments of ``Context.channel_strike_bootstrap``
    and ``fit_channels_along_strike``'s (centre, row, col)."""
    s, where, t = channel_strike.check_args(shape, de, cells, labels, angle, half_length, frequencies, swath, window, step,
                                            max_shift, depth, 0.0, min_samples, min_profiles, with_t=True)
    bl, R, lv, sd, mb = bootstrap.check_resampling(s.de, block_length, replicates, level, seed, min_blocks)
    win_blk_start, blk_hi = strike_bootstrap.blocks_of(t, s.win_lo, s.win_hi, bl)
    nb = int(np.diff(win_blk_start).max(initial=0))
    F = len(s.frequencies)
    if nb * F * 16 > _lib.CHANNEL_STRIKE_BOOT_LDS_TERMS:
        raise ValueError("a window of %d blocks at %d frequencies: its block terms take %d bytes, more than %d - a longer "
                         "block_length or a shorter window" % (nb, F, nb * F * 16, _lib.CHANNEL_STRIKE_BOOT_LDS_TERMS))
    return (Args(s.cells, s.sa, s.ca, s.seg_start, s.seg_label, s.seg_win_start, s.win_lo, s.win_hi, win_blk_start, blk_hi,
                 s.frequencies, s.h, s.w, s.D, s.mode, s.de, s.min_samples, s.min_profiles, mb, R, lv, sd), where)


def _run(ctx, args, where, return_hist, z=None):
    """The call on ``args`` (check_args' record) and its result as ``bootstrap_channels_along_strike`` returns it."""
    rows, hist = ctx.channel_strike_bootstrap(*args, hist=bool(return_hist), z=z)
    out = np.zeros(len(rows), dtype=BOOT_DTYPE)
    for f in rows.dtype.names:
        out[f] = rows[f]
    # (the formulas of fit_channels' table, on rows that carry no cell and no shift: a0 at f0, the widths of the interval)
    full = np.zeros(len(rows), dtype=_lib.PROFILE_SHIFT_DTYPE)
    full["kt"], full["kt_lo"], full["kt_hi"], full["a"] = rows["f0"], rows["f_lo"], rows["f_hi"], rows["a0"]
    derived = channels._table(full, 1, 0.0, 0.0)
    out["depth0"], out["depth_lo"], out["depth_hi"] = derived["depth"], -rows["a_hi"], -rows["a_lo"]
    out["sigma0"], out["width0"], out["curvature0"] = derived["sigma"], derived["width"], derived["curvature"]
    out["width_lo"], out["width_hi"] = derived["width_lo"], derived["width_hi"]
    out["t"], out["row"], out["col"] = where
    return (out, hist) if return_hist else out


def bootstrap_channels_along_strike(data, cells, labels, angle, half_length, frequencies, swath=0, window=None, step=None,
                                    block_length=None, max_shift=0, depth="profile", replicates=1000, level=0.95, seed=0,
                                    min_samples=4, min_profiles=1, min_blocks=5, return_hist=False, device=0):
    """A block-bootstrap interval of the width, the depth and the area at every station along the strike of every reach
    (docs/channels.md, "Intervals per station").

    ``data``, ``cells``, ``labels``, ``angle``, ``half_length``, ``frequencies``, ``swath``, ``window``, ``step``,
    ``max_shift``, ``depth``, ``min_samples`` and ``min_profiles`` are those of ``sl.fit_channels_along_strike``: the
    hand-over, the stations and the windows are its own.  ``block_length``, ``replicates``, ``level``, ``seed`` and
    ``min_blocks`` are those of ``sl.bootstrap_channel_segments``, applied to every window: a cell of a window at
    along-strike coordinate ``t`` lies in block ``floor((t - t_first) / block_length)``, ``t_first`` the window's first
    cell's; replicate 0 takes every block once, each of the others draws as many blocks as the window has, with
    replacement, from the generator of ``bootstrap_along_strike`` keyed by ``seed``, the reach's label and the station, and
    chooses the frequency again by ``bootstrap_channel_segments``' rule of the mode.  Every usable profile keeps the shifts
    it takes on its own: they are not re-fitted per window or per replicate.  A frequency that is dead in a drawn profile is
    dead for that replicate only.  A window with fewer than ``min_blocks`` blocks or fewer than ``min_profiles`` usable
    profiles - an empty one included - is not bootstrapped (``status`` 1, indices -1, NaN floats; 33 where it has both and
    no replicate, replicate 0 included, has a live frequency).  A window's blocks times the frequencies may not exceed 4096.
    Neighbouring stations share profiles where ``step < window``: their intervals are not independent.

    Returns a structured array, one row per (label, station), in ``fit_channels_along_strike``'s order: ``label, station,
    n_cells, n_profiles, n_blocks, replicates, n_failed, f_index0, lo_index, hi_index, status, f0, f_lo, f_hi, a0, a_mean,
    a_sd, a_lo, a_hi, area0, area_mean, area_sd, area_lo, area_hi``, then ``depth0, depth_lo, depth_hi, sigma0, width0,
    width_lo, width_hi, curvature0`` by the formulas of ``sl.fit_channels`` (``width_lo`` from ``f_hi``), then ``t, row,
    col`` as ``fit_channels_along_strike`` reports them.  ``return_hist`` adds the (NW, F) int32 histograms of the indices
    of replicates 1..R.  The replicates themselves are not returned: they would be NW x (R + 1) values.  The same bytes on
    every run."""
    from scarplet_amd import profiles
    z, de = profiles._dem_of(data)
    args, where = check_args(z.shape, de, cells, labels, angle, half_length, frequencies, swath, window, step, block_length,
                             max_shift, depth, replicates, level, seed, min_samples, min_profiles, min_blocks)
    z = np.ascontiguousarray(z, dtype=np.float64)
    from scarplet_amd.core import _context
    return _run(_context(device), args, where, return_hist, z=z)
