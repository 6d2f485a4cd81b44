"""Block-bootstrap intervals of the width, the depth and the area of a reach, on the device (docs/channels.md, "Intervals
per reach").

``fit_channel_segments`` gives a reach one width and an interval that is too narrow: neighbouring profiles sample almost
the same ground, so the pooled degrees of freedom overstate the data - and a reach whose width changes downstream still
gets an interval of one frequency.  ``bootstrap_channel_segments`` resamples blocks of neighbouring profiles along the
strike with replacement, as ``bootstrap_segments`` does for scarps, and chooses the reach's frequency again in every
replicate; the percentiles of the replicates are the interval (sc_channel_bootstrap, include/scarplet_hip.h).
"""
import collections
import math

import numpy as np

from scarplet_amd import _lib, bootstrap, channel_segments, channels

BOOT_FIELDS = [(f, _lib.CHANNEL_BOOT_DTYPE.fields[f][0]) for f in _lib.CHANNEL_BOOT_DTYPE.names] + \
    [(f, np.float64) for f in ("depth0", "depth_lo", "depth_hi", "sigma0", "width0", "width_lo", "width_hi", "curvature0")]
BOOT_DTYPE = np.dtype(BOOT_FIELDS)

# what check_args returns, in the order Context.channel_bootstrap takes it
Args = collections.namedtuple("Args", "cells sa ca seg_start seg_label seg_blk_start blk_start frequencies h w D mode de "
                                      "min_samples min_profiles min_blocks R level seed")


def check_args(shape, de, cells, labels, angle, half_length, frequencies, swath, max_shift, depth, block_length, replicates,
               level, seed, min_samples, min_profiles, min_blocks, seg_strike=None):
    """What the library takes, validated and normalised; ValueError otherwise.  The arguments shared with
    ``fit_channel_segments`` go through ``channel_segments.check_args`` (the park's cap per reach included), those of the
    resampling through ``bootstrap.check_resampling``; the cells are then handed over as ``bootstrap_segments`` hands
    them over (``bootstrap.hand_over``): sorted by (label, block, input position), the blocks cut along the reach's
    strike - the axial mean of its cells' angles, or ``seg_strike`` (the Matcher's ``strike="segment"``)."""
    s = channel_segments.check_args(shape, de, cells, labels, angle, half_length, frequencies, swath, max_shift, depth, 0.0,
                                    min_samples, min_profiles)
    bl, R, lv, sd, mb = bootstrap.check_resampling(s.de, block_length, replicates, level, seed, min_blocks)
    idx, sa, ca, seg_blk_start, blk_start = bootstrap.hand_over(shape, s.de, cells, angle, s, bl, seg_strike)
    return Args(idx, sa, ca, s.seg_start, s.seg_label, seg_blk_start, blk_start, s.frequencies, s.h, s.w, s.D, s.mode, s.de,
                s.min_samples, s.min_profiles, mb, R, lv, sd)


def _run(ctx, args, return_hist, return_replicates, z=None):
    """The call on ``args`` (check_args' record) and its result as ``bootstrap_channel_segments`` returns it."""
    rows, hist, idx, amp = ctx.channel_bootstrap(*args, hist=bool(return_hist), replicates=bool(return_replicates), z=z)
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
    res = [out] + ([hist] if return_hist else []) + ([idx, amp] if return_replicates else [])
    return res[0] if len(res) == 1 else tuple(res)


def area_of(a, f):
    """The area of a trough of depth coefficient ``a`` at frequency ``f``: ``channels._table``'s expression in its order."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return -a / (math.sqrt(np.pi) * f)


def bootstrap_channel_segments(data, cells, labels, angle, half_length, frequencies, swath=0, max_shift=0, depth="profile",
                               block_length=None, replicates=1000, level=0.95, seed=0, min_samples=4, min_profiles=1,
                               min_blocks=5, return_hist=False, return_replicates=False, device=0):
    """A block-bootstrap interval of the width, the depth and the area of every reach (docs/channels.md, "Intervals per
    reach").

    ``data``, ``cells``, ``labels``, ``angle``, ``half_length``, ``frequencies``, ``swath``, ``max_shift``, ``depth``,
    ``min_samples`` and ``min_profiles`` are those of ``sl.fit_channel_segments``; ``block_length`` (required, in data
    units, at least the cell size), ``replicates`` (1..4096), ``level``, ``seed`` and ``min_blocks`` (>= 2) those of
    ``sl.bootstrap_segments``, and so are the blocks - a cell at along-strike coordinate ``t`` lies in block ``floor((t -
    t_min) / block_length)`` of its reach - and the draws.  Every usable profile keeps, at every frequency, the centre shift
    ``fit_channel_segments`` gives it; replicate 0 takes every block once and is that call's ``f_index`` and ``a``; each of
    the others draws as many blocks as the reach has, with replacement, and chooses the frequency again - with
    ``depth="segment"`` the one with the largest ``(sum Sep)^2 / sum See``, with ``depth="profile"`` the one with the
    smallest sum of the profiles' own sse, ``a`` the mean of the drawn profiles' depth coefficients.  A frequency that is
    dead in a drawn profile is dead for that replicate only; a replicate fails only when no frequency is live.

    Returns a structured array, one row per distinct label in ascending order: ``label, n_cells, n_profiles, n_blocks,
    replicates, n_failed, f_index0, lo_index, hi_index, status, f0, f_lo, f_hi, a0, a_mean, a_sd, a_lo, a_hi, area0,
    area_mean, area_sd, area_lo, area_hi`` - ``lo`` and ``hi`` the percentiles ``(1 - level) / 2`` and ``1 - (1 - level) /
    2`` of the replicates, the area ``-a / (sqrt(pi) f)`` taken per replicate - then ``depth0, depth_lo, depth_hi, sigma0,
    width0, width_lo, width_hi, curvature0`` by the formulas of ``sl.fit_channels`` (``width_lo`` from ``f_hi``).
    ``status`` 1: not bootstrapped (fewer than ``min_blocks`` blocks, fewer than ``min_profiles`` usable profiles, or no
    replicate with a live frequency: indices -1, NaN floats; 33 where replicate 0 has none either); else 2 / 4: the
    interval reaches the first / the last frequency.  ``return_hist`` adds the (S, F) int32 histogram of the replicates'
    indices, ``return_replicates`` the (S, R + 1) int8 indices and float64 ``a`` of every replicate, replicate 0 first (-1
    and NaN for a failed one), in that order.  The same bytes on every run."""
    from scarplet_amd import profiles
    z, de = profiles._dem_of(data)
    args = check_args(z.shape, de, cells, labels, angle, half_length, frequencies, swath, max_shift, depth, block_length,
                      replicates, level, seed, min_samples, min_profiles, min_blocks)
    z = np.ascontiguousarray(z, dtype=np.float64)
    from scarplet_amd.core import _context
    return _run(_context(device), args, return_hist, return_replicates, z=z)
