"""Traces of a result: non-maximum suppression, hysteresis and segment labelling on the device (docs/traces.md).

A scarp or a channel shows up in the result planes of ``match`` as a band several cells wide.  ``extract_traces``
thins it across the profile of the template that won each cell, links the thinned cells with hysteresis on the SNR,
labels the 8-connected segments and reduces each to a row of a table - in a few passes over the planes on the device
(sc_trace_planes, include/scarplet_hip.h) instead of a per-row loop on the host.
"""
import collections
import math
import operator

import numpy as np

from scarplet_amd import _lib

Traces = collections.namedtuple("Traces", ["thin", "labels", "segments"])

MAX_CELLS = 2 ** 31 - 1

# the table as Python returns it: the library's row, its label, and what is derived from the sums
SEGMENT_FIELDS = [("label", np.int64)] + [(f, _lib.SEGMENT_DTYPE.fields[f][0]) for f in _lib.SEGMENT_DTYPE.names] + \
    [("mean_amp", np.float64), ("mean_abs_amp", np.float64), ("mean_age", np.float64), ("mean_snr", np.float64),
     ("strike", np.float64)]
SEGMENT_DTYPE = np.dtype(SEGMENT_FIELDS)


def check_args(snr_low, snr_high, min_cells):
    """(snr_low, snr_high, min_cells) validated and normalised; ValueError otherwise."""
    try:
        lo = float(snr_low)
    except (TypeError, ValueError):
        raise ValueError("snr_low must be a number")
    if not (math.isfinite(lo) and lo > 0):
        raise ValueError("snr_low must be finite and > 0, got %r" % (snr_low,))
    if snr_high is None:
        hi = lo
    else:
        try:
            hi = float(snr_high)
        except (TypeError, ValueError):
            raise ValueError("snr_high must be a number")
        if not (math.isfinite(hi) and hi >= lo):
            raise ValueError("snr_high must be finite and >= snr_low, got %r" % (snr_high,))
    if isinstance(min_cells, (bool, np.bool_)):
        raise ValueError("min_cells must be an integer >= 1")
    try:
        mc = operator.index(min_cells)
    except TypeError:
        raise ValueError("min_cells must be an integer >= 1, got %r" % (min_cells,))
    if mc < 1:
        raise ValueError("min_cells must be an integer >= 1, got %r" % (min_cells,))
    return lo, hi, mc


def _planes_of(results):
    """The (4, ny, nx) float64 C-contiguous planes of a result - shapes checked before anything is copied."""
    if isinstance(results, (tuple, list)):
        if len(results) != 4:
            raise ValueError("results must be (amp, age, angle, snr): got %d planes" % len(results))
        planes = [np.asarray(p) for p in results]
        shape = planes[0].shape
        if len(shape) != 2 or any(p.shape != shape for p in planes):
            raise ValueError("results must be four 2-D planes of one shape")
        ny, nx = shape
    else:
        arr = np.asarray(results)
        if arr.ndim != 3 or arr.shape[0] != 4:
            raise ValueError("results must be a (4, ny, nx) array or the 4-tuple of match, got shape %r" % (arr.shape,))
        ny, nx = arr.shape[1:]
        planes = arr
    if ny < 1 or nx < 1:
        raise ValueError("results must have at least one cell")
    if ny * nx > MAX_CELLS:
        raise ValueError("%d x %d cells: more than 2^31 - 1" % (ny, nx))
    if isinstance(planes, list):
        return np.ascontiguousarray(np.stack(planes), dtype=np.float64)
    return np.ascontiguousarray(planes, dtype=np.float64)


def _table(seg):
    """The library's rows -> the Python table (label, the row, means, strike)."""
    out = np.zeros(len(seg), dtype=SEGMENT_DTYPE)
    out["label"] = np.arange(1, len(seg) + 1)
    for f in seg.dtype.names:
        out[f] = seg[f]
    n = seg["n_cells"].astype(np.float64)
    if len(seg):
        out["mean_amp"] = seg["sum_amp"] / n
        out["mean_abs_amp"] = seg["sum_abs_amp"] / n
        out["mean_age"] = seg["sum_age"] / n
        out["mean_snr"] = seg["sum_snr"] / n
        out["strike"] = 0.5 * np.arctan2(seg["sum_sin2a"], seg["sum_cos2a"])
    return out


def _traces(thin, labels, seg):
    return Traces(thin.view(bool), labels, _table(seg))


def extract_traces(results, snr_low, snr_high=None, min_cells=1, device=0):
    """Traces of a result of ``match`` (docs/traces.md).

    ``results``: the (4, ny, nx) array or the (amp, age, angle, snr) tuple of ``sl.match`` - or of the reference, or
    read from a file.  A cell is thinned where it is valid (finite SNR > 0, finite angle) with SNR >= ``snr_low`` and
    is the maximum across the profile of the template that won it; the thinned cells' 8-connected components with
    at least one cell of SNR >= ``snr_high`` (default: ``snr_low``) and at least ``min_cells`` cells are the
    segments, numbered 1..K by their smallest linear index.  Returns ``Traces(thin, labels, segments)``: a bool
    plane, an int32 plane (0 outside segments) and a structured array with one row per segment - ``label``,
    ``first``, ``n_cells``, ``n_strong``, the bounding box, ``peak`` (linear index of the largest SNR) and the planes
    there, the float64 sums, their means and ``strike``, the axial mean orientation.  The same bytes on every run."""
    lo, hi, mc = check_args(snr_low, snr_high, min_cells)
    planes = _planes_of(results)
    from scarplet_amd.core import _context
    return _traces(*_context(device).trace_planes(planes, lo, hi, mc))
