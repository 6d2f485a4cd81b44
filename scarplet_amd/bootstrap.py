"""Block-bootstrap intervals of the age of a trace segment, on the device (docs/bootstrap.md).

``fit_segments`` gives a segment one age and an interval that is too narrow: neighbouring profiles sample almost the
same ground, so the pooled degrees of freedom overstate the data (docs/segments.md).  ``bootstrap_segments`` resamples
blocks of neighbouring profiles along the strike with replacement and re-fits the segment's shared amplitude and age in
every replicate; the percentiles of the replicates' ages and amplitudes are the interval (sc_bootstrap_segments,
include/scarplet_hip.h).
"""
import collections

import numpy as np

from scarplet_amd import _lib, profiles, segments

MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15

BOOT_FIELDS = [(f, _lib.SEGMENT_BOOT_DTYPE.fields[f][0]) for f in _lib.SEGMENT_BOOT_DTYPE.names] + \
    [("height0", np.float64), ("height_lo", np.float64), ("height_hi", np.float64)]
BOOT_DTYPE = np.dtype(BOOT_FIELDS)

# what check_args returns, in the order Context.bootstrap_segments takes it
Args = collections.namedtuple("Args", "cells sa ca seg_start seg_label seg_blk_start blk_start ages h w D de min_samples "
                              "min_profiles min_blocks R level seed")


def mix(z):
    """The splitmix64 finaliser on a Python int, modulo 2^64."""
    z &= MASK64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK64
    z ^= z >> 31
    return z


def draw(seed, label, r, k, nb):
    """The block that draw ``k`` of replicate ``r`` (>= 1) takes in a segment of ``nb`` blocks and label ``label``:
    what the device computes, in Python integers."""
    u = mix(mix((seed ^ (label * GOLDEN)) & MASK64) + ((r << 32) | k))
    return ((u >> 32) * nb) >> 32


def _integer(x, name, lo, hi=None):
    return profiles._integer(x, lo, hi, "%s must be an integer" % name,
                             "%s must lie in %d..%s" % (name, lo, "" if hi is None else hi))


def segment_strikes(angle, seg_start):
    """The axial mean orientation of each segment's cells, ``0.5 atan2(sum sin 2a, sum cos 2a)``: the sums run over the
    segment's cells in the order given (``angle`` grouped by segment, CSR ``seg_start``)."""
    seg = np.repeat(np.arange(len(seg_start) - 1), np.diff(seg_start))
    S = len(seg_start) - 1
    s2 = np.bincount(seg, weights=np.sin(2.0 * angle), minlength=S)
    c2 = np.bincount(seg, weights=np.cos(2.0 * angle), minlength=S)
    return 0.5 * np.arctan2(s2, c2)


def blocks_of(cells, nx, de, strike, seg_start, block_length):
    """The block of every cell, ``cells`` grouped by segment (CSR ``seg_start``), ``strike`` one per segment: the
    along-strike coordinate ``t = de (row cos a_s + col sin a_s)`` - the profile runs along (row, col) = (-sin a,
    cos a), this is its normal - and ``floor((t - t_min) / block_length)``, ``t_min`` the segment's smallest."""
    n = np.diff(seg_start)
    a = np.repeat(strike, n)
    t = de * ((cells // nx).astype(np.float64) * np.cos(a) + (cells % nx).astype(np.float64) * np.sin(a))
    if len(t) == 0:
        return np.zeros(0, dtype=np.int64)
    full = np.flatnonzero(n > 0)
    tmin = np.zeros(len(n))
    tmin[full] = np.minimum.reduceat(t, seg_start[:-1][full])
    return np.floor((t - np.repeat(tmin, n)) / block_length).astype(np.int64)


def check_resampling(de, block_length, replicates, level, seed, min_blocks):
    """The rules of the resampling, shared with ``strike_bootstrap``: ``block_length`` required, a finite number of at
    least the cell size ``de``; ``replicates`` an integer in 1..4096, ``min_blocks`` one of at least 2, ``seed`` one in
    0..2^64 - 1; ``level`` strictly between 0 and 1.  Returns (block_length, R, level, seed, min_blocks)."""
    if block_length is None:
        raise ValueError("block_length is required: the length of a block along the strike, in data units")
    bl = profiles._number(block_length, "block_length")
    if bl < de:
        raise ValueError("block_length must be at least the cell size %r, got %r" % (de, block_length))
    R = _integer(replicates, "replicates", 1, _lib.BOOT_MAX_REPLICATES)
    mb = _integer(min_blocks, "min_blocks", 2)
    sd = _integer(seed, "seed", 0, MASK64)
    lv = profiles._number(level, "level")
    if not 0.0 < lv < 1.0:
        raise ValueError("level must lie strictly between 0 and 1, got %r" % (level,))
    return bl, R, lv, sd, mb


def check_args(shape, de, cells, labels, angle, half_length, swath, block_length, replicates, level, seed, ages,
               min_samples, min_profiles, min_blocks, max_shift, seg_strike=None):
    """What the library takes, validated and normalised; ValueError otherwise.  The arguments shared with
    ``fit_segments`` go through ``segments.check_args``.  The cells are then sorted by (label, block, input position),
    all stable, and the blocks that hold a cell are numbered along the strike.  ``seg_strike``: the strike of label L
    at index L - 1 (the Matcher's ``strike="segment"``) instead of the axial mean of the cells' angles.  Returns
    (cells, sa, ca, seg_start, seg_label, seg_blk_start, blk_start, ages, h, w, D, de, min_samples, min_profiles,
    min_blocks, R, level, seed)."""
    # (the park is checked as sc_fit_segments_shift counts it)
    s = segments.check_args(shape, de, cells, labels, angle, half_length, swath, ages, 0.0, min_samples, min_profiles, shift=True)
    idx, sa, ca, seg_start, seg_label, de, h, ms = s.cells, s.sa, s.ca, s.seg_start, s.seg_label, s.de, s.h, s.min_samples
    D = profiles.check_shift(max_shift, False, de, h, ms)
    D = 0 if D is None else D
    bl, R, lv, sd, mb = check_resampling(de, block_length, replicates, level, seed, min_blocks)
    idx, sa, ca, seg_blk_start, blk_start = hand_over(shape, de, cells, angle, s, bl, seg_strike)
    return Args(idx, sa, ca, seg_start, seg_label, seg_blk_start, blk_start, s.ages, h, s.w, D, de, ms, s.min_profiles, mb, R,
                lv, sd)


def hand_over(shape, de, cells, angle, s, block_length, seg_strike=None):
    """The hand-over of a block bootstrap, shared with ``channel_bootstrap``: ``s`` is the record of a segment call's
    ``check_args`` (cells, sa, ca, seg_start, seg_label, order, kept) on the caller's ``cells`` and ``angle``.  The strike
    of a segment is the axial mean of its cells' angles, or ``seg_strike`` (the strike of label L at index L - 1); the
    cells are sorted by (label, block, input position), all stable, and the blocks that hold a cell are numbered along the
    strike.  Returns (cells, sa, ca, seg_blk_start, blk_start)."""
    idx, sa, ca, seg_start, seg_label = s.cells, s.sa, s.ca, s.seg_start, s.seg_label
    ny, nx = (int(v) for v in shape)
    if seg_strike is None:
        pick = s.kept[s.order]
        a = profiles._angles_of(angle, profiles._cells_of(cells, ny, nx), ny, nx)[pick]
        strike = segment_strikes(a, seg_start)
    else:
        strike = np.asarray(seg_strike, dtype=np.float64)[seg_label.astype(np.int64) - 1]
    blk = blocks_of(idx, nx, de, strike, seg_start, block_length)
    seg = np.repeat(np.arange(len(seg_label)), np.diff(seg_start))
    by = np.lexsort((blk, seg))                                        # (stable: input order is kept within a block)
    idx, sa, ca, blk = idx[by], sa[by], ca[by], blk[by]
    first = np.ones(len(idx), dtype=bool)                               # the first cell of every block that holds one
    first[1:] = (seg[1:] != seg[:-1]) | (blk[1:] != blk[:-1])
    blk_start = np.concatenate([np.flatnonzero(first), [len(idx)]]).astype(np.int64)
    seg_blk_start = np.searchsorted(blk_start[:-1], seg_start).astype(np.int64)
    return np.ascontiguousarray(idx), np.ascontiguousarray(sa), np.ascontiguousarray(ca), seg_blk_start, blk_start


def bootstrap_segments(data, cells, labels, angle, half_length, swath=0, block_length=None, replicates=1000, level=0.95,
                       seed=0, ages=None, min_samples=4, min_profiles=1, min_blocks=5, max_shift=None, return_hist=False,
                       return_replicates=False, device=0):
    """A block-bootstrap interval of the age and the amplitude of every segment (docs/bootstrap.md).

    ``data``, ``cells``, ``labels``, ``angle``, ``half_length``, ``swath``, ``ages``, ``min_samples``, ``min_profiles``
    and ``max_shift`` are those of ``sl.fit_segments``.  The cells of a segment are cut into blocks along its strike (the
    axial mean of its cells' angles): a cell at along-strike coordinate ``t`` lies in block ``floor((t - t_min) /
    block_length)``; ``block_length`` is required, in data units, at least the cell size, and must exceed the
    correlation length of the residuals along the strike.  Replicate 0 takes every block once; each of the
    ``replicates`` (1..4096) others draws as many blocks as the segment has, with replacement, from a counter-based
    generator keyed by ``seed`` and the segment's label, and re-fits the shared amplitude and the age.  A segment with
    fewer than ``min_blocks`` (>= 2) blocks or fewer than ``min_profiles`` usable profiles is not bootstrapped
    (``status`` 1, indices -1, NaN floats).

    Returns a structured array, one row per distinct label in ascending order: ``label, n_cells, n_profiles, n_blocks,
    replicates, n_failed, kt_index0, lo_index, hi_index, status, kt0, kt_lo, kt_hi, a0, a_mean, a_sd, a_lo, a_hi,
    height0, height_lo, height_hi`` (heights = 2 a) - ``lo`` and ``hi`` the percentiles ``(1 - level) / 2`` and
    ``1 - (1 - level) / 2`` of the replicates.  ``return_hist`` adds the (S, A) int32 histogram of the replicates' age
    indices, ``return_replicates`` the (S, R + 1) int8 indices and float64 amplitudes of every replicate, replicate 0
    first (-1 and NaN for a failed one), in that order.  The same bytes on every run."""
    z, de = profiles._dem_of(data)
    args = check_args(z.shape, de, cells, labels, angle, half_length, swath, block_length, replicates, level, seed, ages,
                      min_samples, min_profiles, min_blocks, max_shift)
    z = np.ascontiguousarray(z, dtype=np.float64)
    from scarplet_amd.core import _context
    return _run(_context(device), args, return_hist, return_replicates, z=z)


def _run(ctx, args, return_hist, return_replicates, z=None):
    rows, hist, idx, amp = ctx.bootstrap_segments(*args, hist=bool(return_hist), replicates=bool(return_replicates), z=z)
    out = np.zeros(len(rows), dtype=BOOT_DTYPE)
    for f in rows.dtype.names:
        out[f] = rows[f]
    out["height0"] = 2.0 * rows["a0"]
    out["height_lo"] = 2.0 * rows["a_lo"]
    out["height_hi"] = 2.0 * rows["a_hi"]
    res = [out] + ([hist] if return_hist else []) + ([idx, amp] if return_replicates else [])
    return res[0] if len(res) == 1 else tuple(res)
