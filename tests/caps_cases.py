"""The per-cell calls at the top of their accepted ranges: the inputs of tests/test_caps_host.py and tests/test_gpu_caps.py.

include/scarplet_hip.h caps the per-cell calls - half-length 1024, swath 32, 64 ages or frequencies, centre shift 64, ramp
half-width 64, lateral lag 255 with a band of 64 lines out to 1024 cells, 64 robust iterations, 4096 replicates.  The cases
here sit ON those caps, with at most 8 cells or stations each; the restatements they are compared with are the existing
ones (lateral_reference, shift_reference, ramp_reference, channel_reference, profile_reference, segment_ramp_reference,
bootstrap_reference, robust_reference) with their own tolerances.  CPU and numpy only, every input seeded.

With fewer than 100 cells TIE_SHARE allows no tie, so the restatement's own decisions must stand clear: ``margins`` /
``lateral_margins`` measure by how much, and tests/test_caps_host.py asserts MARGIN on every case."""
import os
import re
import time

import numpy as np

import channel_reference as cr
import lateral_reference as lr
import profile_reference as pr
import ramp_reference as rr
import shift_reference as sh

MARGIN = 1e-6                                    # a decision of a restatement is clear when it is decided by more, relatively
AGES64 = 10 ** np.linspace(0, 3.4, 64)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "scarplet_hip.h")


def header_caps():
    """The integer ``#define SC_...`` of include/scarplet_hip.h by name."""
    with open(HEADER) as f:
        return {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (SC_\w+)[ \t]+(\d+)[ \t]*(?:/\*.*)?$", f.read(), re.M)}


def _cells(v):
    return np.ascontiguousarray(v, dtype=np.int64)


def _angles(a, cells):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), np.shape(cells)))


_KEPT, SECONDS = {}, {}


def kept(key, make):
    """make() once per process: the DEMs and the restatements are shared by the tests and left unchanged.  SECONDS[key] is
    what make() took."""
    if key not in _KEPT:
        t0 = time.perf_counter()
        _KEPT[key] = make()
        SECONDS[key] = time.perf_counter() - t0
    return _KEPT[key]


# ---- 1, 2: sl.lateral_offsets ------------------------------------------------------------------------------------------------
LATERAL_SHAPE, LATERAL_SEED = (2700, 2200), 1
# (h, D, q0, q1, min_samples) in cells.  The first is every cap at once; the others one cap at a time, and D = 127 and 128 -
# 255 and 257 lags - either side of a boundary between two rounds of 64 ranks
LATERAL_ALL = (1024, 255, 961, 1024, 8)
LATERAL_ONE = [(1024, 0, 1, 1, 8), (5, 255, 2, 9, 4), (40, 31, 961, 1024, 8), (40, 127, 2, 9, 8), (40, 128, 2, 9, 8)]
LATERAL_ANGLES = np.array([0.0, 0.03, -0.02, 0.01])


def lateral_dem():
    return kept("lateral dem", lambda: lr.rough_dem(LATERAL_SHAPE, LATERAL_SEED))


def lateral_stations():
    """Three stations near the centre, whose profiles and bands lie inside the grid at every cap, and a corner, which stays
    unfitted."""
    ny, nx = LATERAL_SHAPE
    r0, c0 = ny // 2, nx // 2
    return _cells([r0 * nx + c0, (r0 + 7) * nx + c0 - 11, (r0 - 5) * nx + c0 + 9, (ny - 1) * nx + nx - 1]), LATERAL_ANGLES.copy()


def lateral_lds_bytes(h, D, waves=4):
    """The dynamic LDS k_lt_fit asks for: u, v and the mse curve of every wave, in doubles."""
    return 8 * waves * ((2 * h + 1) + (2 * (h + D) + 1) + (2 * D + 1))


def lateral_ref(p):
    h, D, q0, q1, ms = p
    cells, ang = lateral_stations()
    return kept(("lateral", p), lambda: lr.lateral_offsets(lateral_dem(), 1.0, cells, ang, h, q0, q1, D, 1.0, ms))


def lateral_margins(ref):
    """(the smallest relative gap between the best and the second-best mse, the smallest relative distance of a curve value
    from thr) over the fitted stations of a lateral restatement."""
    rows, mse, thr = ref
    gap = near = np.inf
    for k in np.flatnonzero(rows["status"] != 1):
        m = np.sort(mse[k][~np.isnan(mse[k])])
        if len(m) > 1:
            gap = min(gap, (m[1] - m[0]) / m[0])
        near = min(near, float(np.min(np.abs(m - thr[k]) / thr[k])))
    return gap, near


def rounds_of(lags):
    """The round of 64 ranks in which each lag is tried (lateral_reference.shift_of's order: 0, -1, +1, ...)."""
    lags = np.asarray(lags, dtype=np.int64)
    return np.where(lags < 0, -2 * lags - 1, 2 * lags) // 64


# ---- margins of a (cells x ages x candidates) restatement ---------------------------------------------------------------------
def margins(grid, curve, dof, delta, keys=None, scale=None):
    """How clear the decisions of one restated cell are, each as the smallest relative difference: 'pick' (per age or
    frequency: the best candidate's key against the second best; ``keys`` defaults to ``grid``, the differences are taken
    relative to ``scale`` or else to the best key), 'best' (the best age against the second best on ``curve``) and 'walk'
    (every curve value against thr).  NaN entries are no candidates."""
    keys = grid if keys is None else keys
    pick = np.inf
    for row in np.asarray(keys, dtype=np.float64):
        v = np.sort(row[np.isfinite(row)])
        if len(v) > 1:
            pick = min(pick, (v[1] - v[0]) / (v[0] if scale is None else scale))
    c = np.sort(curve[np.isfinite(curve)])
    best = (c[1] - c[0]) / c[0] if len(c) > 1 else np.inf
    thr = c[0] * (1.0 + delta / dof)
    return {"pick": float(pick), "best": float(best), "walk": float(np.min(np.abs(c[1:] - thr) / thr)) if len(c) > 1 else np.inf}


def least(ms):
    """The smallest of each margin over the cells' ``margins``."""
    return {k: min(m[k] for m in ms) for k in ("pick", "best", "walk")}


# ---- 3: the centre shift at D = 64 -------------------------------------------------------------------------------------------
SHIFT_OFFSETS = np.array([0, -20, 35, -50, 60, -64, 64, 80])              # columns off the scarp's line
SHIFT_ROWS = 156 + 36 * np.arange(8)                                     # (rows of ramp_reference.line_cells)


def shift_case():
    """Eight cells of synthetic_z(600) off the scarp's line by SHIFT_OFFSETS columns: the step sits about -offset cos(0.2)
    cells along the profile, the last one past the range."""
    z = kept("synthetic 600", lambda: pr.synthetic_z(600))
    line = rr.line_cells(600)                                            # rows 150, 153, ...
    cells = _cells(line[(SHIFT_ROWS - 150) // 3] + SHIFT_OFFSETS)
    return dict(name="shift D64 A64 h160", z=z, de=1.0, cells=cells, angle=_angles(0.2, cells), h=160, w=2, D=64, ages=AGES64,
                delta=1.0, min_samples=15)


def shift_ref():
    c = shift_case()
    return kept("shift ref", lambda: sh.fit_profiles(c["z"], c["de"], c["cells"], c["angle"], c["h"], c["w"], c["D"], c["ages"],
                                                     c["delta"], c["min_samples"]))


def shift_margins(ref, delta=1.0):
    return least([margins(r["grid"], r["curve"], r["dof"], delta) for r in ref if r["status"] != 1])


def spread_of(shifts, D):
    """What the winners of a shifted case must cover: |d| >= 3 D / 4 of both signs and |d| = D."""
    d = np.asarray(shifts, dtype=np.int64)
    return bool((d >= (3 * D) // 4).any() and (d <= -((3 * D) // 4)).any() and (np.abs(d) == D).any())


# ---- 4: the ramp at M = 64 ---------------------------------------------------------------------------------------------------
RAMP_ROWS = np.array([180, 225, 270, 315, 360, 405])


def ramp_case(L=40):
    """Six cells on the line of a ramp of half-width L cells diffused for AGES64[20]; the given slope of the run in that
    mode is the surface's own, |b + a / L| with a = 1 and b = -0.01."""
    z = kept(("ramp", L), lambda: rr.ramp_scarp(600, float(AGES64[20]), float(L), noise=0.02))
    cells = _cells(rr.line_cells(600)[(RAMP_ROWS - 150) // 3])
    return dict(name="ramp M64 A64 h160 L%d" % L, z=z, de=1.0, cells=cells, angle=_angles(0.2, cells), h=160, w=2, M=64,
                ages=AGES64, delta=1.0, min_samples=15, slope=abs(-0.01 + 1.0 / L))


def ramp_ref(L, mode):
    c = ramp_case(L)
    return kept(("ramp ref", L, mode), lambda: rr.restate(c, mode))


def ramp_margins(ref, mode, slope, delta=1.0):
    out = []
    for r in ref:
        if r["status"] != 1:
            keys = np.where(np.isinf(r["keys"]), np.nan, r["keys"])
            out.append(margins(r["grid"], r["curve"], r["dof"], delta, keys, slope if mode == rr.SLOPE else None))
    return least(out)


# ---- 5: sl.fit_channels ------------------------------------------------------------------------------------------------------
def channel_cases():
    """'D64 F64 h160': eight cells of channel_z(600) off the thalweg by SHIFT_OFFSETS; 'h1024 F8 D2': four cells on the
    thalweg of a 2400 x 2400 trough."""
    z = kept("channel 600", lambda: cr.channel_z(600))
    cells = _cells(cr.line_cells(600, 600, SHIFT_ROWS) + SHIFT_OFFSETS)
    a = dict(name="channel D64 F64 h160", z=z, de=1.0, cells=cells, angle=_angles(0.2, cells), h=160, w=2, D=64,
             frequencies=cr.freqs_of_sigma(np.geomspace(3.0, 15.0, 64)), delta=1.0, min_samples=15)
    zb = kept("channel 2400", lambda: cr.channel_z(2400))
    cells = _cells(cr.line_cells(2400, 2400, np.array([1100, 1180, 1260, 1340])) + np.array([0, 1, -1, 2]))
    b = dict(name="channel h1024 F8 D2", z=zb, de=1.0, cells=cells, angle=_angles(0.2, cells), h=1024, w=1, D=2,
             frequencies=cr.freqs_of_sigma(np.geomspace(3.0, 14.0, 8)), delta=1.0, min_samples=100)
    return {"D64": a, "h1024": b}


def channel_margins(ref, delta=1.0):
    return least([margins(r["grid"], r["curve"], r["dof"], delta) for r in ref if not r["status"] & 1])


# ---- 6: a swath of 32 --------------------------------------------------------------------------------------------------------
def swath_case():
    """sl.fit_profiles with 65 lines a point: eight cells on the scarp's line of a 400 x 400 surface - five in the interior,
    one six rows from the top, whose swath leaves the grid, and two next to a block of NaN cells."""
    from scarplet_amd import _plan

    def make():
        z = pr.synthetic_z(400, seed=11).copy()
        z[236:244, 200:215] = np.nan
        return z
    z = kept("swath dem", make)
    rows = np.array([6, 90, 130, 170, 200, 228, 250, 330])
    cells = _cells(_line(400, rows))
    return dict(name="swath 32 h30 A35", z=z, de=1.0, cells=cells, angle=_angles(0.2, cells), h=30, w=32,
                ages=np.asarray(_plan.age_grid(), dtype=np.float64), delta=1.0, min_samples=15, sample=None)


def _line(n, rows, theta=0.2):
    """The cell of each row in ``rows`` on the scarp's line of synthetic_z(n) (ramp_reference.line_cells for any rows)."""
    x = np.linspace(-n / 2, n / 2, num=n)
    rows = np.asarray(rows)
    yrot = -x[None, :] * np.cos(theta) + x[rows][:, None] * np.sin(theta)
    return rows.astype(np.int64) * n + np.argmin(np.abs(yrot), axis=1)


def swath_ref():
    return kept("swath ref", lambda: pr.restate(swath_case())[1])


def swath_margins(ref, delta=1.0):
    return least([margins(r["curve"][None, :], r["curve"], r["n"] - 3, delta) for r in ref if r["status"] != 1])


# ---- 7: the segment fits at the caps -----------------------------------------------------------------------------------------
def segment_shift_case():
    """The cells of shift_case() as two segments, their cells interleaved."""
    return dict(shift_case(), name="segments D64", labels=np.array([3, 7, 3, 7, 3, 7, 3, 7], dtype=np.int64), min_profiles=1)


def segment_shift_ref(shifts):
    """shift_reference.fit_segments of segment_shift_case() with the (K, A) shifts ``shifts``."""
    c = segment_shift_case()
    return sh.fit_segments(c["z"], c["de"], c["cells"], c["labels"], c["angle"], c["h"], c["w"], c["D"], c["ages"], shifts,
                           c["delta"], c["min_samples"], c["min_profiles"])


def segment_margins(ref, delta=1.0):
    """'best' and 'walk' of the segments' sse curves (their 'pick' is the single profiles')."""
    ms = [margins(r["curve"][None, :], r["curve"], r["dof"], delta) for r in ref if r["status"] != 1]
    return {k: v for k, v in least(ms).items() if k != "pick"}


def segment_ramp_case(L=40):
    """The cells of ramp_case(L) as two segments, their cells interleaved."""
    return dict(ramp_case(L), name="segments M64 L%d" % L, labels=np.array([5, 2, 5, 2, 5, 2], dtype=np.int64), min_profiles=1)


def segment_ramp_ref(L, mode):
    import segment_ramp_reference as sx
    c = segment_ramp_case(L)
    return kept(("segment ramp ref", L, mode), lambda: sx.restate(c, mode))


def segment_ramp_margins(ref, mode, slope, delta=1.0):
    out = []
    for r in ref:
        if r["status"] != 1:
            keys = np.where(np.isinf(r["keys"]), np.nan, r["keys"])
            out.append(margins(r["grid"], r["curve"], r["dof"], delta, keys, slope if mode == rr.SLOPE else None))
    return least(out)


# ---- 8: sl.bootstrap_segments at R = 4096 ------------------------------------------------------------------------------------
def bootstrap_case():
    """bootstrap_reference's "nb 1 4 5 70" with SC_BOOT_MAX_REPLICATES replicates."""
    import bootstrap_reference as br
    base = [c for c in br.gpu_cases() if c["name"] == "nb 1 4 5 70"][0]
    return dict(base, name="nb 1 4 5 70, R 4096", R=4096)


def bootstrap_ref():
    import bootstrap_reference as br
    return kept("bootstrap ref", lambda: br.restate(bootstrap_case()))


STRIKE_BOOT_LDS_BYTES = 16 * 4096 + 9 * 8192                             # what sc_strike_bootstrap.hip keeps in LDS at R = 4096


# ---- 9: robust=, 64 iterations -----------------------------------------------------------------------------------------------
ROBUST_T = (64, 32, 16)
ROBUST_AGES = np.array([3.0, 10.0, 30.0, 100.0])


def robust_case(loss, T):
    """Six cells on the scarp's line of robust_reference's pit surface, four ages, h = 100, T reweightings."""
    import robust_reference as ro
    z = kept("pit surface", lambda: ro.pit_surface()[0])
    cells = _cells(rr.line_cells(600)[[5, 20, 35, 50, 65, 80]])
    return ro.case("robust %s T%d" % (loss, T), z, 1.0, cells, 0.2, 100, 2, ages=ROBUST_AGES, ms=15, robust=loss, iterations=T)


def robust_refs(loss, T):
    """(the float64 restatement's rows, the longdouble one's) of robust_case(loss, T)."""
    import robust_reference as ro
    c = robust_case(loss, T)
    return kept(("robust ref", loss, T), lambda: (ro.restate(c), ro.restate(c, fit=ro.wfit_longdouble, cond=False)))


def robust_disagreement(loss, T):
    """The largest difference between the two restatements, scaled as robust_reference.compare_rows scales: the loss curve,
    the sse and the scale relative, the coefficients of every age over the profile's range (b times h de)."""
    c = robust_case(loss, T)
    worst = 0.0
    for a, b in zip(*robust_refs(loss, T)):
        if a["status"] & 1 or b["status"] & 1 or not np.array_equal(np.isnan(a["curve"]), np.isnan(b["curve"])):
            return np.inf
        live = ~np.isnan(a["curve"])
        worst = max(worst, float(np.max(np.abs(a["curve"][live] - b["curve"][live]) / b["curve"][live])),
                    abs(a["sse"] - b["sse"]) / b["sse"], abs(a["scale"] - b["scale"]) / b["scale"])
        d = np.abs(a["coefs"][live] - b["coefs"][live]) * np.array([1.0, c["h"] * c["de"], 1.0])
        worst = max(worst, float(d.max()) / a["ptp"])
        if (a["kt_index"], a["lo_index"], a["hi_index"], a["n_down"], a["ls_index"]) != \
                (b["kt_index"], b["lo_index"], b["hi_index"], b["n_down"], b["ls_index"]):
            return np.inf
    return worst


def robust_iterations(loss, limit):
    """(T, the disagreement at that T): the largest T of ROBUST_T at which the float64 and the longdouble restatement
    agree within ``limit``; (None, the disagreement at the smallest T) where none does."""
    d = np.inf
    for T in ROBUST_T:
        d = robust_disagreement(loss, T)
        if d <= limit:
            return T, d
    return None, d


def robust_margins(ref, delta=1.0):
    out = []
    for r in ref:
        if not r["status"] & 1:
            m = margins(r["sse0"][None, :], r["curve"], r["n"] - 3, delta)   # ('pick': the least-squares index)
            out.append(m)
    return least(out)
