"""One scarp age per trace segment, fitted jointly on the device (docs/segments.md).

``fit_profiles`` dates every cell of a trace on its own; a mapped scarp gets ONE age with ONE interval.
``fit_segments`` cuts the same profiles (the same samples, bit for bit) and solves, per segment and age, one
least-squares problem over all of them: the amplitude ``a`` and the age are the segment's, every profile keeps an
intercept and a far-field slope of its own, since elevation and slope vary along the strike (sc_fit_segments,
include/scarplet_hip.h).
"""
import collections

import numpy as np

from scarplet_amd import _lib, profiles

# the tables as Python returns them
FIT_FIELDS = [(f, _lib.SEGMENT_FIT_DTYPE.fields[f][0]) for f in _lib.SEGMENT_FIT_DTYPE.names] + [("height", np.float64)]
FIT_DTYPE = np.dtype(FIT_FIELDS)
CELL_FIELDS = [("row", np.int64), ("col", np.int64)] + \
    [(f, _lib.SEGMENT_CELL_DTYPE.fields[f][0]) for f in _lib.SEGMENT_CELL_DTYPE.names] + [("label", np.int32)]
CELL_DTYPE = np.dtype(CELL_FIELDS)
# ... and with max_shift: each profile's shift at the segment's best age, in cells and in data units
SHIFT_CELL_FIELDS = CELL_FIELDS[:-1] + [("shift_index", np.int32), ("shift", np.float64), ("label", np.int32)]
SHIFT_CELL_DTYPE = np.dtype(SHIFT_CELL_FIELDS)
# ... and with max_width: the half-width of the segment's initial ramp, in cells and in data units, and its gradient
RAMP_FIT_FIELDS = FIT_FIELDS[:-1] + [("width_index", np.int32), ("width", np.float64), ("initial_slope", np.float64),
                                     ("height", np.float64)]
RAMP_FIT_DTYPE = np.dtype(RAMP_FIT_FIELDS)
# ... and with weights or a robust loss: the loss and the scale of the best age, the points it down-weighted, the best age
# before the robust step and the profiles the last iterate left dormant; per cell its share of the loss, its down-weighted
# points and whether it was dormant
ROBUST_FIT_FIELDS = FIT_FIELDS[:-1] + [("loss", np.float64), ("scale", np.float64), ("n_down", np.int32), ("ls_index", np.int32),
                                       ("n_dormant", np.int32), ("height", np.float64)]
ROBUST_FIT_DTYPE = np.dtype(ROBUST_FIT_FIELDS)
ROBUST_CELL_FIELDS = CELL_FIELDS[:-1] + [("loss", np.float64), ("n_down", np.int32), ("dormant", np.int32), ("label", np.int32)]
ROBUST_CELL_DTYPE = np.dtype(ROBUST_CELL_FIELDS)
# ... and with refine: the minimum and the interval off the grid, after ``height``; per cell its slope, intercept and share
# of the sse at ``kt_fine``
FINE_FIT_FIELDS = FIT_FIELDS + [(f, np.float64) for f in _lib.SEGMENT_FINE_FLOATS] + [("height_fine", np.float64),
                                                                                      ("status_fine", np.int32)]
FINE_FIT_DTYPE = np.dtype(FINE_FIT_FIELDS)
FINE_CELL_FIELDS = CELL_FIELDS[:-1] + [(f, np.float64) for f in _lib.SEGMENT_FINE_CELL_FLOATS] + [("label", np.int32)]
FINE_CELL_DTYPE = np.dtype(FINE_CELL_FIELDS)

# what check_args returns: the arguments of Context.fit_segments in its order, then the sort's permutation of the kept
# cells and their input positions
Args = collections.namedtuple("Args", "cells sa ca seg_start seg_label ages h w de delta min_samples min_profiles order kept")


def _labels_of(labels, idx, ny, nx):
    """One int64 label per cell: one per cell, or an (ny, nx) int plane read at the cells."""
    lab = np.asarray(labels)
    if lab.size and lab.dtype.kind not in "iu":
        raise ValueError("labels must be integers, got %s" % lab.dtype)
    if lab.ndim == 2:
        if lab.shape != (ny, nx):
            raise ValueError("a label plane must have the grid's shape %r, got %r" % ((ny, nx), lab.shape))
        lab = lab.ravel()[idx]
    elif lab.ndim != 1 or len(lab) != len(idx):
        raise ValueError("labels must be one integer per cell (%d) or an (ny, nx) plane" % len(idx))
    lab = lab.astype(np.int64)
    if lab.size and lab.max() > 2 ** 31 - 1:
        raise ValueError("labels must fit 32 bits")
    return lab


def check_args(shape, de, cells, labels, angle, half_length, swath, ages, delta, min_samples, min_profiles, shift=False):
    """What the library takes, validated and normalised; ValueError otherwise.  The shared arguments go through
    ``profiles.check_args``; cells of label <= 0 are dropped, the rest grouped by label with a stable sort (input
    order is kept within a label).  Returns (cells, sa, ca, seg_start, seg_label, ages, h, w, de, delta, min_samples,
    min_profiles, order, kept): the first three sorted, ``kept`` the input positions of the cells that stay and
    ``order`` the sort's permutation of them.  ``shift``: the call parks each cell's shifts too (max_shift is given)."""
    idx, sa, ca, kt, h, w, de, d, ms = profiles.check_args(shape, de, cells, angle, half_length, swath, ages, delta,
                                                           min_samples)
    ny, nx = (int(v) for v in shape)
    lab = _labels_of(labels, idx, ny, nx)
    mp = profiles._integer(min_profiles, 1, None, "min_profiles must be an integer >= 1", "min_profiles must be an integer >= 1")
    kept = np.flatnonzero(lab > 0)
    order = np.argsort(lab[kept], kind="stable")
    pick = kept[order]
    seg_label, counts = np.unique(lab[kept], return_counts=True)
    seg_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    _check_cap(seg_start, _lib.SEGMENT_MAX_PARK // (8 * ((2 * h + 1) + 4 * len(kt)) + (len(kt) if shift else 0)),
               " and number of ages")
    return Args(np.ascontiguousarray(idx[pick]), np.ascontiguousarray(sa[pick]), np.ascontiguousarray(ca[pick]), seg_start,
                np.ascontiguousarray(seg_label, dtype=np.int32), kt, h, w, de, d, ms, mp, order, kept)


def _check_cap(seg_start, cap, what):
    """ValueError for a segment (CSR ``seg_start``) of more than ``cap`` cells; ``what``: the option that set the cap."""
    counts = np.diff(seg_start)
    if len(counts) and counts.max() > cap:
        raise ValueError("a segment of %d cells: more than %d at this half_length%s" % (counts.max(), cap, what))


def check_park(args, M):
    """The park cap of a call with ``max_width``: 8 ((2h + 1) + 4 A (M + 1)) bytes per cell, a segment at a time
    (sc_fit_segments_ramp).  ``args`` as check_args returns them; ValueError for a segment above the cap."""
    _check_cap(args.seg_start, _lib.SEGMENT_MAX_PARK // (8 * ((2 * args.h + 1) + 4 * len(args.ages) * (M + 1))),
               ", number of ages and max_width")


def check_robust_park(args, plane):
    """The park cap of a call with ``weights`` or ``robust``: 8 ((2h + 1)(1 + plane) + 9 A) bytes per cell, a segment at a
    time (sc_fit_segments_robust; ``_lib.segment_robust_cap``).  ``args`` as check_args returns them; ValueError for a
    segment above the cap."""
    _check_cap(args.seg_start, _lib.segment_robust_cap(args.h, len(args.ages), plane),
               " and number of ages with weights or robust")


def check_refine(args, refine, max_shift=None, weights=None, robust=None, max_width=None):
    """``profiles.check_refine`` for the joint fit: None, or R; the park - 8 ((2h + 1) + 4 (A + 128)) bytes per cell with
    R > 0, a segment at a time (sc_fit_segments_refine; ``_lib.segment_refine_cap``) - must hold every segment.  ``args`` as
    check_args returns them; ValueError otherwise."""
    R = profiles.check_refine(refine, max_shift, weights, robust, max_width)
    if R is not None:
        _check_cap(args.seg_start, _lib.segment_refine_cap(args.h, len(args.ages), R), " and number of ages with refine")
    return R


def check_robust(shape, args, weights, robust, tuning, iterations, robust_scale, max_shift, max_width):
    """``profiles.check_robust`` for the joint fit: None, or (plane or None, loss, k, T, sigma or 0.0); neither option is
    built together with ``max_shift`` or ``max_width``, and the park must hold every segment.  ValueError otherwise."""
    if (weights is not None or robust is not None) and max_width is not None:
        raise ValueError("weights and robust are not built together with max_width")
    rb = profiles.check_robust(shape, weights, robust, tuning, iterations, robust_scale, max_shift)
    if rb is not None:
        check_robust_park(args, rb[0] is not None)
    return rb


def check_options(shape, args, max_shift, return_shift, weights, robust, tuning, iterations, robust_scale, max_width,
                  initial_slope, return_width, refine):
    """The options of ``fit_segments`` beside ``args`` (check_args' record), checked in the one order that decides which
    ValueError a doubly wrong call gets: ``profiles.Options(shift, robust, ramp, refine)``, every park checked."""
    D = profiles.check_shift(max_shift, return_shift, args.de, args.h, args.min_samples)
    rb = check_robust(shape, args, weights, robust, tuning, iterations, robust_scale, max_shift, max_width)
    rp = profiles.check_width(max_width, initial_slope, return_width, args.de, args.h, args.min_samples, max_shift)
    if rp is not None:
        check_park(args, rp[0])
    return profiles.Options(D, rb, rp, check_refine(args, refine, max_shift, weights, robust, max_width))


def fit_segments(data, cells, labels, angle, half_length, swath=0, ages=None, delta=1.0, min_samples=4,
                 min_profiles=1, return_cells=False, return_curve=False, device=0, max_shift=None, return_shift=False,
                 max_width=None, initial_slope=None, return_width=False, weights=None, robust=None, tuning=None,
                 iterations=8, robust_scale=None, refine=None):
    """Fit ONE diffusion scarp per segment to the profiles cut across the strike at its cells (docs/segments.md).

    ``data``, ``cells``, ``angle``, ``half_length``, ``swath``, ``ages``, ``delta`` and ``min_samples`` are those of
    ``sl.fit_profiles``.  ``labels``: one int per cell, or an (ny, nx) int plane read at the cells (the ``labels`` of
    ``extract_traces``); the cells of one label are one segment, cells of label <= 0 are dropped.  Per segment and
    age the usable profiles (at least ``min_samples`` valid points on either side) are fitted together by
    ``c0_c + b_c s + a erf(s / (2 sqrt(kt)))``: ``a`` and ``kt`` shared, an intercept and a slope per profile.  The
    age with the smallest pooled sum of squared residuals wins; ``lo_index .. hi_index`` is the run of ages around it
    whose sse stays within ``sse_min (1 + delta / dof)``, ``dof = n - 2 n_profiles - 1``.  A segment with fewer than
    ``min_profiles`` usable profiles has ``status`` 1 and NaN fields.

    Returns a structured array, one row per distinct label in ascending order: ``label, n_cells, n_profiles, n, dof,
    kt_index, lo_index, hi_index, status, kt, kt_lo, kt_hi, a, sse, rmse, height`` (= 2 a).  ``return_cells`` adds
    the per-cell table in input order (``row, col, cell, used, n, b, c0, sse, label``: each profile's slope,
    intercept and sse at the segment's best age) and ``return_curve`` the (S, A) sse curves, in that order.  The
    same bytes on every run.

    ``max_shift`` (data units; None: every step stays at its cell) gives every profile a shift of its own, chosen at
    every age as ``sl.fit_profiles(..., max_shift=...)`` chooses it; the joint fit then has each profile's erf moved by
    its shift.  ``dof`` loses one more per profile when the range is not 0, ``status`` gains 8 where a usable profile's
    shift at the best age is the end of the range, the cell table gains ``shift_index`` and ``shift``, and
    ``return_shift`` adds the (K, A) int8 plane of every cell's shift at every age, in input order, last.

    ``max_width`` (data units; None: the scarp starts as a vertical step) fits the scarp that started as a ramp of
    half-width ``L = m de``, ``m <= floor(max_width / de)`` cells, the model of ``sl.fit_profiles(..., max_width=...)``
    with the half-width shared by the segment like the amplitude and the age (docs/segments.md, "The initial slope").
    With ``initial_slope=None`` the width is free: every age takes the ``m`` of its smallest pooled sse, and one degree of
    freedom goes to the width.  With ``initial_slope`` (a gradient magnitude, > 0) every age takes the ``m >= 1`` whose
    ``|bbar + a / (m de)|`` is nearest to it, ``bbar`` the mean far-field slope of the segment's profiles.  The table
    gains ``width_index``, ``width`` (m de) and ``initial_slope`` (signed; +-inf at ``m = 0``) ahead of ``height``, the
    curves are the chosen pairs' sse, ``status`` gains 8 where ``width_index`` is the end of the range, and
    ``return_width`` adds the (S, A) int8 plane of every age's m, last.  Not built together with ``max_shift``.

    ``weights``, ``robust``, ``tuning``, ``iterations`` and ``robust_scale`` are those of ``sl.fit_profiles``: a weight on
    every point of every sum, and ``iterations`` rounds of iteratively reweighted least squares per age under the Huber or
    the Tukey loss, on ONE scale per segment - ``robust_scale``, or 1.4826 times the median of the pooled absolute
    residuals of the least-squares fit at its best age (docs/segments.md, "Weights and robust fits").  A profile that the
    Tukey loss leaves with fewer than ``min_samples`` weighted points on a side is dormant: it has no say in the shared
    amplitude until it wakes.  The choice and the interval run on the robust loss; the table gains ``loss``, ``scale``,
    ``n_down``, ``ls_index`` and ``n_dormant`` ahead of ``height``, the cell table ``loss``, ``n_down`` and ``dormant``,
    ``status`` 16 marks a segment without a scale (the least-squares row) and ``1 | 32`` one none of whose ages survived, and
    ``return_curve`` returns the loss curves.  Not built together with ``max_shift`` or ``max_width``.

    ``refine`` (None: the age is one of the grid; 0, 1 or 2) is that of ``sl.fit_profiles`` on the segment's pooled sse: that
    many levels of 64 candidate ages of the segment's own bracket below the grid, for the minimum and for either end of the
    interval, every candidate fitted jointly (docs/segments.md, "Continuous ages").  Every field of the plain tables and the
    curves keep the plain call's bytes; the table gains ``kt_fine, kt_lo_fine, kt_hi_fine, a_fine, sse_fine`` (<= ``sse``),
    ``rmse_fine, height_fine, status_fine`` after ``height`` and the cell table ``b_fine, c0_fine, sse_fine`` ahead of
    ``label``.  Not built together with ``max_shift``, ``max_width``, ``weights`` or ``robust``."""
    z, de = profiles._dem_of(data)
    args = check_args(z.shape, de, cells, labels, angle, half_length, swath, ages, delta, min_samples, min_profiles,
                      shift=max_shift is not None)
    opts = check_options(z.shape, args, max_shift, return_shift, weights, robust, tuning, iterations, robust_scale, max_width,
                         initial_slope, return_width, refine)
    z = np.ascontiguousarray(z, dtype=np.float64)
    from scarplet_amd.core import _context
    return _run(_context(device), args, z.shape[1], return_cells, return_curve, z=z, return_shift=return_shift,
                return_width=return_width, **opts._asdict())


def _run(ctx, args, nx, return_cells, return_curve, z=None, shift=None, return_shift=False, ramp=None, return_width=False,
         robust=None, refine=None):
    """The call the options name, on ``args`` (check_args' record), and its result as ``fit_segments`` returns it: the table,
    then what was asked for of the cell table, the curves, the shifts and the widths - per cell in input order."""
    call, de, order = args[:-2], args.de, args.order       # (the call takes all but order and kept)
    out = dict(cell_table=bool(return_cells), curve=bool(return_curve), z=z)
    plane = None
    fit_dtype = ROBUST_FIT_DTYPE if robust is not None else RAMP_FIT_DTYPE if ramp is not None else FIT_DTYPE
    cell_dtype = ROBUST_CELL_DTYPE if robust is not None else CELL_DTYPE if shift is None else SHIFT_CELL_DTYPE
    if refine is not None:
        rows, tab, curve = ctx.fit_segments_refine(*call, refine, **out)
        fit_dtype, cell_dtype = FINE_FIT_DTYPE, FINE_CELL_DTYPE
    elif robust is not None:
        wt, loss, k, T, sigma = robust
        rows, tab, curve = ctx.fit_segments_robust(*call, weights=wt, loss=loss, tuning=k, iterations=T, scale=sigma, **out)
    elif ramp is not None:
        M, mode, slope = ramp
        rows, tab, curve, widths = ctx.fit_segments_ramp(*call, M, mode=mode, slope=slope, width_plane=bool(return_width), **out)
    elif shift is None:
        rows, tab, curve = ctx.fit_segments(*call, **out)
    else:
        rows, tab, curve, plane = ctx.fit_segments(*call, shift=shift, shift_plane=bool(return_shift), **out)
    table = np.zeros(len(rows), dtype=fit_dtype)
    for f in rows.dtype.names:
        table[f] = rows[f]
    table["height"] = 2.0 * rows["a"]
    if refine is not None:
        table["height_fine"] = 2.0 * rows["a_fine"]
    res = [table]
    if return_cells or return_shift:
        back = np.empty(len(order), dtype=np.int64)                    # sorted position of each kept cell
        back[order] = np.arange(len(order))
    if return_cells:
        ct = np.zeros(len(tab), dtype=cell_dtype)
        for f in tab.dtype.names:
            ct[f] = tab[f][back]
        ct["row"] = ct["cell"] // nx
        ct["col"] = ct["cell"] % nx
        ct["label"] = np.repeat(args.seg_label, np.diff(args.seg_start))[back]
        if shift is not None:
            ct["shift"] = np.where(np.isnan(ct["b"]), np.nan, ct["shift_index"] * de)
        res.append(ct)
    if return_curve:
        res.append(curve)
    if return_shift:
        res.append(np.ascontiguousarray(plane[back]))
    if return_width:
        res.append(widths)
    return res[0] if len(res) == 1 else tuple(res)
