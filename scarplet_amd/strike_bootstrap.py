"""Block-bootstrap intervals of the offset and the age at every station along a trace, on the device (docs/strike.md,
"Intervals per station").

``fit_along_strike`` gives the offset ``2 a`` and the age ``kt`` as functions of the position along a trace, each with
``fit_segments``' pooled interval - too narrow, because neighbouring profiles are not independent (docs/segments.md).
``bootstrap_segments`` has the usable interval, but for a whole segment.  ``bootstrap_along_strike`` is the two together:
in every window of ``fit_along_strike`` the blocks of neighbouring profiles along the strike are resampled with
replacement and the window's shared amplitude and age are re-fitted in every replicate (sc_strike_bootstrap,
include/scarplet_hip.h).  The windows and the blocks are cut here, in float64 numpy, and handed over as integers.
"""
import collections

import numpy as np

from scarplet_amd import _lib, bootstrap, strike

MASK64 = bootstrap.MASK64
STATION = 0xD1B54A32D192ED03

BOOT_FIELDS = [(f, _lib.STRIKE_BOOT_DTYPE.fields[f][0]) for f in _lib.STRIKE_BOOT_DTYPE.names] + \
    [(f, np.float64) for f in ("height0", "height_lo", "height_hi", "t", "row", "col")]
BOOT_DTYPE = np.dtype(BOOT_FIELDS)

# the first of what check_args returns, in the order Context.strike_bootstrap takes it
Args = collections.namedtuple("Args", "cells sa ca seg_start seg_label seg_win_start win_lo win_hi win_blk_start blk_hi ages "
                              "h w D de min_samples min_profiles min_blocks R level seed")


def draw(seed, label, station, r, k, nb):
    """The block that draw ``k`` of replicate ``r`` (>= 1) takes in the window ``station`` of the segment ``label``, a
    window of ``nb`` blocks: what the device computes, in Python integers.  Station 0 has ``bootstrap.draw``'s key."""
    key = bootstrap.mix((seed ^ (label * bootstrap.GOLDEN) ^ (station * STATION)) & MASK64)
    u = bootstrap.mix(key + ((r << 32) | k))
    return ((u >> 32) * nb) >> 32


def blocks_of(t, win_lo, win_hi, block_length):
    """The blocks of every window ``[win_lo, win_hi)`` of cells at ``t`` (ascending within a segment): the block of a cell
    is ``floor((t_c - t_first) / block_length)``, ``t_first`` the ``t`` of the window's first cell
    (``bootstrap.blocks_of`` applied to the window), and the blocks that hold a cell are numbered along the strike.  All
    in float64.  Returns (win_blk_start, blk_hi), int64: the CSR array of the windows over the blocks and the end cell
    of every block."""
    t = np.asarray(t, dtype=np.float64)
    win_lo = np.asarray(win_lo, dtype=np.int64)
    win_hi = np.asarray(win_hi, dtype=np.int64)
    n = win_hi - win_lo
    NW = len(n)
    total = int(n.sum())
    if total == 0:
        return np.zeros(NW + 1, dtype=np.int64), np.zeros(0, dtype=np.int64)
    w = np.repeat(np.arange(NW), n)                                     # the window of every (window, cell) pair
    cell = np.arange(total) - np.repeat(np.cumsum(n) - n, n) + np.repeat(win_lo, n)
    b = np.floor((t[cell] - np.repeat(t[np.minimum(win_lo, len(t) - 1)], n)) / block_length).astype(np.int64)
    first = np.ones(total, dtype=bool)                                  # the first cell of every block that holds one
    first[1:] = (w[1:] != w[:-1]) | (b[1:] != b[:-1])
    at = np.flatnonzero(first)
    last = np.concatenate([at[1:], [total]]) - 1                        # a block ends where the next one, or the window's, begins
    blk_hi = (cell[last] + 1).astype(np.int64)
    win_blk_start = np.concatenate([[0], np.cumsum(np.bincount(w[at], minlength=NW))]).astype(np.int64)
    return win_blk_start, np.ascontiguousarray(blk_hi)


def check_args(shape, de, cells, labels, angle, half_length, swath, window, step, block_length, replicates, level, seed,
               ages, min_samples, min_profiles, min_blocks, max_shift):
    """What the library takes, validated and normalised; ValueError otherwise.  Everything shared with
    ``fit_along_strike`` goes through ``strike.handover`` (``segments.check_args``, ``profiles.check_shift``, the rules of
    the window and the step), the resampling through ``bootstrap.check_resampling``.  The blocks of every window are
    then cut (``blocks_of``); a window whose block terms do not fit 64 KiB - ``nb A 16 > 65536`` - is refused.
    Returns (cells, sa, ca, seg_start, seg_label, seg_win_start, win_lo, win_hi, win_blk_start, blk_hi, ages, h, w, D, de,
    min_samples, min_profiles, min_blocks, R, level, seed) and ``fit_along_strike``'s (centre, row, col)."""
    s, where, t = strike.handover(shape, de, cells, labels, angle, half_length, swath, window, step, ages, 0.0, min_samples,
                                  min_profiles, max_shift)
    bl, R, lv, sd, mb = bootstrap.check_resampling(s.de, block_length, replicates, level, seed, min_blocks)
    win_blk_start, blk_hi = blocks_of(t, s.win_lo, s.win_hi, bl)
    nb = int(np.diff(win_blk_start).max(initial=0))
    A = len(s.ages)
    if nb * A * 16 > _lib.STRIKE_BOOT_LDS_TERMS:
        raise ValueError("a window of %d blocks at %d ages: its block terms take %d bytes, more than %d - a longer "
                         "block_length or a shorter window" % (nb, A, nb * A * 16, _lib.STRIKE_BOOT_LDS_TERMS))
    return (Args(s.cells, s.sa, s.ca, s.seg_start, s.seg_label, s.seg_win_start, s.win_lo, s.win_hi, win_blk_start, blk_hi,
                 s.ages, s.h, s.w, s.D, s.de, s.min_samples, s.min_profiles, mb, R, lv, sd), where)


def bootstrap_along_strike(data, cells, labels, angle, half_length, swath=0, window=None, step=None, block_length=None,
                           replicates=1000, level=0.95, seed=0, ages=None, min_samples=4, min_profiles=1, min_blocks=5,
                           max_shift=None, return_hist=False, device=0):
    """A block-bootstrap interval of the offset and the age at every station along the strike of every segment
    (docs/strike.md, "Intervals per station").

    ``data``, ``cells``, ``labels``, ``angle``, ``half_length``, ``swath``, ``window``, ``step``, ``ages``,
    ``min_samples``, ``min_profiles`` and ``max_shift`` are those of ``sl.fit_along_strike``: the hand-over, the stations
    and the windows are its own.  ``block_length``, ``replicates``, ``level``, ``seed`` and ``min_blocks`` are those of
    ``sl.bootstrap_segments``, applied to every window: a cell of a window at along-strike coordinate ``t`` lies in block
    ``floor((t - t_first) / block_length)``, ``t_first`` the window's first cell's; replicate 0 takes every block once,
    each of the others draws as many blocks as the window has, with replacement, from the generator of
    ``bootstrap_segments`` keyed by ``seed``, the segment's label and the station.  A window with fewer than
    ``min_blocks`` blocks or fewer than ``min_profiles`` usable profiles - an empty one included - is not bootstrapped
    (``status`` 1, indices -1, NaN floats).  A window's blocks times the ages may not exceed 4096.

    Returns a structured array, one row per (label, station), in ``fit_along_strike``'s order: ``label, station,
    n_cells, n_profiles, n_blocks, replicates, n_failed, kt_index0, lo_index, hi_index, status, kt0, kt_lo, kt_hi, a0,
    a_mean, a_sd, a_lo, a_hi, height0, height_lo, height_hi`` (heights = 2 a), ``t, row, col`` as ``fit_along_strike``
    reports them.  ``return_hist`` adds the (NW, A) int32 histograms of the replicates' age indices.  The replicates
    themselves are not returned: they would be NW x (R + 1) values.  The same bytes on every run."""
    from scarplet_amd import profiles
    z, de = profiles._dem_of(data)
    args, where = check_args(z.shape, de, cells, labels, angle, half_length, swath, window, step, block_length, replicates,
                             level, seed, ages, min_samples, min_profiles, min_blocks, max_shift)
    z = np.ascontiguousarray(z, dtype=np.float64)
    from scarplet_amd.core import _context
    return _run(_context(device), args, where, return_hist, z=z)


def _run(ctx, args, where, return_hist, z=None):
    rows, hist = ctx.strike_bootstrap(*args, hist=bool(return_hist), z=z)
    out = np.zeros(len(rows), dtype=BOOT_DTYPE)
    for f in rows.dtype.names:
        out[f] = rows[f]
    out["height0"] = 2.0 * rows["a0"]
    out["height_lo"] = 2.0 * rows["a_lo"]
    out["height_hi"] = 2.0 * rows["a_hi"]
    out["t"], out["row"], out["col"] = where
    return (out, hist) if return_hist else out
