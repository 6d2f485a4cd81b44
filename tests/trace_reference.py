"""Float64 numpy restatement of the traces of a result (docs/traces.md, include/scarplet_hip.h sc_trace_planes):
thinning across the winning template's profile, 8-connected segments with hysteresis, the segment table.  What the
device's sc_trace_* is checked against; not a test module."""
import numpy as np
from scipy import ndimage

PI = 3.141592653589793
# (drow, dcol) per sector: along the profile of the template that won the cell (alpha = -angle, y along the rows)
STEPS = ((0, 1), (1, -1), (1, 0), (1, 1))

SUM_FIELDS = ("sum_amp", "sum_abs_amp", "sum_age", "sum_snr", "sum_cos2a", "sum_sin2a")
INT_FIELDS = ("first", "n_cells", "n_strong", "row_min", "row_max", "col_min", "col_max", "peak")
PEAK_FIELDS = ("snr_peak", "amp_peak", "age_peak", "angle_peak")


def valid(ang, snr):
    with np.errstate(invalid="ignore"):
        return np.isfinite(snr) & (snr > 0) & np.isfinite(ang) & (np.abs(ang) <= 1e6)


def sectors(ang):
    """0..3 per cell (cells whose angle is not finite: 0, never used)."""
    a = np.where(np.isfinite(ang) & (np.abs(ang) <= 1e6), ang, 0.0)
    q = np.floor((a / PI) * 4.0 + 0.5)
    return (q - 4.0 * np.floor(q / 4.0)).astype(np.int64)


def _shifted(v, dr, dc):
    """out[r, c] = v[r + dr, c + dc] inside the grid, -inf outside."""
    ny, nx = v.shape
    out = np.full_like(v, -np.inf)
    rs, re = max(0, -dr), min(ny, ny - dr)
    cs, ce = max(0, -dc), min(nx, nx - dc)
    if rs < re and cs < ce:
        out[rs:re, cs:ce] = v[rs + dr:re + dr, cs + dc:ce + dc]
    return out


def thin(ang, snr, snr_low):
    v = np.where(np.isfinite(snr), snr, -np.inf)
    s = sectors(ang)
    ok = valid(ang, snr)
    with np.errstate(invalid="ignore"):
        ok &= snr >= snr_low
    out = np.zeros(snr.shape, dtype=bool)
    for k, (dr, dc) in enumerate(STEPS):
        m = ok & (s == k)
        with np.errstate(invalid="ignore"):
            out |= m & (snr > _shifted(v, -dr, -dc)) & (snr >= _shifted(v, dr, dc))
    return out


def trace(planes, snr_low, snr_high=None, min_cells=1):
    """(thin bool, labels int32, table: dict of field -> array, one entry per segment in label order)."""
    amp, age, ang, snr = (np.asarray(p, dtype=np.float64) for p in planes)
    snr_high = snr_low if snr_high is None else snr_high
    t = thin(ang, snr, snr_low)
    comp, nc = ndimage.label(t, structure=np.ones((3, 3), dtype=int))
    flat = comp.ravel()
    idx = np.flatnonzero(flat)
    cl = flat[idx]
    with np.errstate(invalid="ignore"):
        strong = (snr.ravel()[idx] >= snr_high)
    n_cells = np.bincount(cl, minlength=nc + 1)
    n_strong = np.bincount(cl, weights=strong, minlength=nc + 1).astype(np.int64)
    first = np.full(nc + 1, np.iinfo(np.int64).max)
    np.minimum.at(first, cl, idx)
    keep = (n_strong >= 1) & (n_cells >= min_cells)
    keep[0] = False
    kept = np.flatnonzero(keep)
    kept = kept[np.argsort(first[kept], kind="stable")]
    relabel = np.zeros(nc + 1, dtype=np.int64)
    relabel[kept] = np.arange(1, len(kept) + 1)
    labels = relabel[flat].reshape(snr.shape).astype(np.int32)
    return t, labels, table(amp, age, ang, snr, labels, strong_of=lambda ii: snr.ravel()[ii] >= snr_high)


def table(amp, age, ang, snr, labels, strong_of):
    nx = labels.shape[1]
    lab = labels.ravel()
    idx = np.flatnonzero(lab)
    order = np.lexsort((idx, lab[idx]))
    idx = idx[order]
    L = lab[idx]
    K = int(lab.max()) if lab.size else 0
    out = {}
    if K == 0:
        for f in INT_FIELDS:
            out[f] = np.zeros(0, dtype=np.int64)
        for f in PEAK_FIELDS + SUM_FIELDS:
            out[f] = np.zeros(0)
        return out
    starts = np.flatnonzero(np.r_[True, L[1:] != L[:-1]])
    a, g, an, s = (p.ravel()[idx] for p in (amp, age, ang, snr))
    r, c = idx // nx, idx % nx
    out["first"] = idx[starts].astype(np.int64)
    out["n_cells"] = np.diff(np.r_[starts, len(idx)]).astype(np.int64)
    out["n_strong"] = np.add.reduceat(strong_of(idx).astype(np.int64), starts)
    out["row_min"] = np.minimum.reduceat(r, starts)
    out["row_max"] = np.maximum.reduceat(r, starts)
    out["col_min"] = np.minimum.reduceat(c, starts)
    out["col_max"] = np.maximum.reduceat(c, starts)
    # peak: the largest snr, ties to the smallest index (cells are in index order inside a segment)
    pk_order = np.lexsort((idx, -s, L))
    pk_first = pk_order[np.flatnonzero(np.r_[True, L[pk_order][1:] != L[pk_order][:-1]])]
    peak = idx[pk_first]
    out["peak"] = peak.astype(np.int64)
    out["snr_peak"] = snr.ravel()[peak]
    out["amp_peak"] = amp.ravel()[peak]
    out["age_peak"] = age.ravel()[peak]
    out["angle_peak"] = ang.ravel()[peak]
    for name, v in (("sum_amp", a), ("sum_abs_amp", np.abs(a)), ("sum_age", g), ("sum_snr", s),
                    ("sum_cos2a", np.cos(2.0 * an)), ("sum_sin2a", np.sin(2.0 * an))):
        out[name] = np.add.reduceat(v, starts)
        out[name + "_abs"] = np.add.reduceat(np.abs(v), starts)     # the scale of each sum's rounding
    return out
