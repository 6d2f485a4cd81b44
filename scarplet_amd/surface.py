"""The search's float64 SNR surface at chosen cells, on the device (docs/surface.md).

``sl.match`` tells per cell which (age, orientation) scored best.  ``snr_surface`` returns, for the cells one asks about,
the float64 score of every template of the grid - the misfit surface Hilley et al. 2010 read their age ranges from - and
what it says about the maximum: the run of ages and the run of orientations whose best score stays within ``drop`` of it,
and how many templates do (sc_snr_surface, include/scarplet_hip.h).  It works for every template class a search takes.
"""
import numpy as np

from scarplet_amd import _lib, _plan, profiles

MAX_CELLS = 2 ** 31 - 1

FIELDS = [("row", np.int64), ("col", np.int64), ("cell", np.int64), ("par_index", np.int32), ("ang_index", np.int32),
          ("par", np.float64), ("angle", np.float64), ("amp", np.float64), ("snr", np.float64),
          ("par_lo_index", np.int32), ("par_hi_index", np.int32), ("par_lo", np.float64), ("par_hi", np.float64),
          ("ang_lo_index", np.int32), ("ang_hi_index", np.int32), ("angle_lo", np.float64), ("angle_hi", np.float64),
          ("n_within", np.int32), ("status", np.int32)]
DTYPE = np.dtype(FIELDS)


def _grid_axis(values, name):
    try:
        v = np.atleast_1d(np.asarray(values, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError("%s must be numbers" % name)
    if v.ndim != 1:
        raise ValueError("%s must be a 1-D sequence" % name)
    if v.size and not np.all(np.isfinite(v)):
        raise ValueError("%s must be finite" % name)
    return np.ascontiguousarray(v)


def check_args(shape, cells, params, angles, drop):
    """(cells as int64 linear indices, params, angles, keep) validated; ValueError otherwise.  ``params=None`` and
    ``angles=None`` are the grids of ``sl.match``; ``keep = 1.0 - drop``, formed here once."""
    ny, nx = (int(v) for v in shape)
    if ny < 2 or nx < 2:
        raise ValueError("the grid must be at least 2 x 2, got %d x %d" % (ny, nx))
    d = profiles._number(drop, "drop")
    if not 0.0 <= d < 1.0:
        raise ValueError("drop must lie in [0, 1), got %r" % (drop,))
    par = _grid_axis(_plan.age_grid() if params is None else params, "the parameters (ages)")
    ang = _grid_axis(_plan.angle_grid() if angles is None else angles, "angles")
    if par.size == 0 or ang.size == 0:
        raise ValueError("an empty grid: %d parameters x %d orientations" % (par.size, ang.size))
    if par.size * ang.size > _lib.SURFACE_MAX_TEMPLATES:
        raise ValueError("%d x %d templates: more than %d" % (par.size, ang.size, _lib.SURFACE_MAX_TEMPLATES))
    idx = profiles._cells_of(cells, ny, nx)
    if len(idx) > MAX_CELLS:
        raise ValueError("%d cells: more than 2^31 - 1" % len(idx))
    return idx, par, ang, 1.0 - d


def table(rows, idx, nx, params, angles, label=None):
    """The library's rows -> the Python table: where the cell lies, the indices, and the grid's values at them (NaN where
    the index is -1); ``label`` when given."""
    out = np.zeros(len(rows), dtype=np.dtype(FIELDS + ([] if label is None else [("label", np.int32)])))
    out["row"], out["col"], out["cell"] = idx // nx, idx % nx, idx
    for f in ("par_index", "ang_index", "amp", "snr", "n_within", "status"):
        out[f] = rows[f]
    out["par_lo_index"], out["par_hi_index"] = rows["par_lo"], rows["par_hi"]
    out["ang_lo_index"], out["ang_hi_index"] = rows["ang_lo"], rows["ang_hi"]
    for dst, src, grid in (("par", "par_index", params), ("par_lo", "par_lo", params), ("par_hi", "par_hi", params),
                           ("angle", "ang_index", angles), ("angle_lo", "ang_lo", angles), ("angle_hi", "ang_hi", angles)):
        k = rows[src]
        out[dst] = np.where(k >= 0, grid[np.maximum(k, 0)], np.nan)
    if label is not None:
        out["label"] = label
    return out


def _refuse_nan():
    raise ValueError("the DEM has NaN cells: every score would be NaN (as in the reference); fill them first "
                     "(DEMGrid._fill_nodata)")


def run(m, Template, scale, params, angles, traces_or_cells, drop, return_surface, kwargs):
    """Matcher.snr_surface: the checks, the descriptors, the call, the table."""
    from scarplet_amd import traces
    from scarplet_amd.core import _refuse_crater
    _refuse_crater(Template)
    if not getattr(m, "whole", False):
        raise ValueError("snr_surface needs the whole DEM on the device, not a block of it")
    if getattr(m, "nan_dem", False):
        _refuse_nan()
    label = None
    cells = traces_or_cells
    if isinstance(traces_or_cells, traces.Traces):
        labels = np.asarray(traces_or_cells.labels)
        if labels.shape != (m.ny, m.nx):
            raise ValueError("the traces' planes must have the DEM's shape %r" % ((m.ny, m.nx),))
        cells = np.flatnonzero(labels.ravel() > 0)
        label = labels.ravel()[cells]
    idx, par, ang, keep = check_args((m.ny, m.nx), cells, params, angles, drop)
    K, n_par, n_ang = len(idx), len(par), len(ang)
    if K == 0:
        rows = np.zeros(0, dtype=_lib.SURFACE_ROW_DTYPE)
        cube = np.zeros((0, n_par, n_ang))
        out = table(rows, idx, m.nx, par, ang, label)
        return (out, cube, cube.copy()) if return_surface else out
    arr = m.describe(Template, scale, par, ang, **kwargs)[0]
    rc = np.column_stack([idx // m.nx, idx % m.nx]).astype(np.int32)
    rows, snr, amp = m.ctx.snr_surface(arr, n_par, n_ang, rc, keep, surface=bool(return_surface))
    out = table(rows, idx, m.nx, par, ang, label)
    if not return_surface:
        return out
    # the library's cubes are orientation-major, as the templates are handed over: (K, n_ang, n_par)
    return out, np.ascontiguousarray(snr.transpose(0, 2, 1)), np.ascontiguousarray(amp.transpose(0, 2, 1))


def snr_surface(data, Template, cells, scale, ages=None, angles=None, drop=0.1, return_surface=False, device=0, **kwargs):
    """The float64 SNR of every (age, orientation) template at ``cells``, and the templates the surface does not tell
    apart from the best (docs/surface.md).

    ``data``: the DEMGrid (uploaded).  ``Template``: any class a search takes - the built-in ones, the UpperBreak
    classes, plugins (``**kwargs`` reach the class); not ``Crater``.  ``cells``: linear indices ``r * nx + c``, a ``(rows,
    cols)`` tuple or a bool plane; repeats are allowed and the output is in input order.  ``ages`` / ``angles``: the grid
    (default: ``10 ** arange(0, 3.5, 0.1)`` and the 181 orientations of ``sl.match``).  Per cell ``S[ia, ib]`` is
    ``match_template()``'s SNR of template (age ia, orientation ib) in float64.  Templates are compared orientation-major,
    ages inner, a NaN counting as -inf; the first maximum gives ``par_index, ang_index, par, angle, snr, amp``.  With
    ``thr = snr * (1 - drop)``: ``par_lo_index .. par_hi_index`` is the run of ages around the best whose score, maximised
    over the orientations, stays ``>= thr``; ``ang_lo_index .. ang_hi_index`` likewise over the orientations (it does not
    wrap); ``n_within`` counts the templates ``>= thr``.  ``status`` 1: no template scores above 0 at the cell (it lies
    outside every template's window limits) - indices -1, NaN floats; else the sum of 2 / 4 (the age interval touches the
    young / old end of the grid) and 8 / 16 (the orientation interval touches the first / last orientation).  ``drop`` is a
    relative criterion on the SNR, not a calibrated confidence level.

    Returns a structured array, one row per cell: ``row, col, cell, par_index, ang_index, par, angle, amp, snr,
    par_lo_index, par_hi_index, par_lo, par_hi, ang_lo_index, ang_hi_index, angle_lo, angle_hi, n_within, status`` - and with
    ``return_surface`` the (K, n_par, n_ang) float64 cubes of snr and amp.  The same bytes on every run."""
    from scarplet_amd.core import Matcher, _grid_of, _refuse_crater
    _refuse_crater(Template)
    try:
        z = _grid_of(data)[0]
    except AttributeError:
        raise ValueError("data must be a DEMGrid")
    if np.isnan(z).any():
        _refuse_nan()
    check_args(z.shape, cells, ages, angles, drop)
    m = Matcher(data, device=device)
    try:
        return run(m, Template, scale, ages, angles, cells, drop, return_surface, kwargs)
    finally:
        m.ctx.clear_windows()
